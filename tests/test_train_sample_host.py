"""--device-training-sample, the parts that need no GPU: the flag and its keys, eligibility of the
'sample' topology, the sampling of a round (the active nodes draw the CPU path's batches from the
CPU path's RNG stream, inactive nodes draw nothing), the per-row `first` flags of the momentum
step, and the argument checks of niidmix_sample_step_mean_update_f32."""
import json
import os
import re

import pytest
import torch

import test_eval_gnlenet_host as th
from conftest import REPO

SAMPLE = "device-training-sample"
GN = "device-training-gn-lenet"
ROUNDS = 9                      # 50 samples in batches of 16: an epoch is 4 rounds of one node


class Net(torch.nn.Module):
    """The linear model of tests/test_train_host.py; forward notes the marker of every sample."""

    def __init__(self, k=6, c=3):
        super().__init__()
        self.fc = torch.nn.Linear(k, c)
        self.seen = []

    def forward(self, x, params):
        self.seen.append(x[:, 0].tolist())
        return torch.nn.functional.log_softmax(self.fc(x.view(-1, self.fc.in_features)), dim=1)


def _params(**alg):
    a = {"learning-rate": 0.1, "learning-momentum": 0.0, "batch-size": 16, "initial-averaging": False,
         "clique-gradient": False, "unbiased-gradient": False, "device-training": True, SAMPLE: True}
    a.update(alg)
    return {"meta": {"log": "WARNING"}, "algorithm": a, "logger": {},
            "topology": {"name": "sample", "sample-method": "random-with-overlap", "sample-size": 3,
                         "sample-overlap": 1}}


def _nodes(params, n=6, samples=50):
    from niidmix import d_sgd
    nodes = []
    for r in range(n):
        # sample j of node r carries the marker value 1000 r + j in every feature
        ts = [(torch.full((6,), float(1000 * r + j)), j % 3) for j in range(samples)]
        mdl = Net()
        nodes.append({"rank": r, "epoch": 0, "train-set": ts, "model": mdl,
                      "optimizer": d_sgd.optimizer(mdl, params)})
    return nodes


def _topo():
    return {"edges": {}, "weights": []}


def test_cli_flag_writes_both_keys(tmp_path, monkeypatch):
    from niidmix import d_sgd
    for argv, want in (([], (None, None, None)),
                       (["--device-training-sample"], (True, True, None)),
                       (["--device-training-sample", "--device-training-gn-lenet"], (True, True, True)),
                       (["--device-training"], (True, None, None))):
        run = tmp_path / ("run%d" % len(argv) + ("p" if argv == ["--device-training"] else ""))
        run.mkdir()
        (run / "params.json").write_text(json.dumps({"topology": {"name": "sample"}}))
        monkeypatch.setattr(d_sgd, "load_topology", lambda rundir: _topo())
        d_sgd.main(["--rundir", str(run)] + argv)
        alg = json.loads((run / "params.json").read_text())["algorithm"]
        assert (alg.get("device-training"), alg.get(SAMPLE), alg.get(GN)) == want, argv


def test_sample_is_accepted_under_the_key_only(monkeypatch):
    from niidmix import d_sgd, train
    monkeypatch.setattr(d_sgd, "_sample_cache", {})
    p = _params()
    assert train.sample_run(p)
    assert train.check_eligible(_nodes(p), p, _topo()) == (6, 3)
    state, step, done = d_sgd.init(_nodes(p), _topo(), p)
    assert state["step"] == 0 and state["topology"] == _topo()
    idx = next(state["nodes"][0]["train-iterator"])
    assert idx.dtype == torch.int64 and idx.dim() == 1               # index loaders
    # the gradient-averaging flags are ignored, as in the reference's sample branch: no lists, no
    # 'cliques' / 'neighbourhoods' needed
    for key in ("clique-gradient", "unbiased-gradient"):
        q = _params(**{key: True})
        assert train.check_eligible(_nodes(q), q, _topo()) == (6, 3)
        d_sgd.init(_nodes(q), _topo(), q)
    # without the key: the refusal of before, which may name the new flag
    for off in ({SAMPLE: False}, {SAMPLE: False, GN: True}):
        q = _params(**off)
        q["algorithm"].pop(SAMPLE)
        with pytest.raises(ValueError, match="'sample' topology") as e:
            train.check_eligible(_nodes(q), q, _topo())
        assert ("--device-training-gn-lenet" if GN in off else "--device-training ") in str(e.value)
        with pytest.raises(ValueError, match="'sample' topology"):
            d_sgd.init(_nodes(q), _topo(), q)
    # the key on another topology changes nothing: the graph round's refusals and lists
    q = _params(**{"clique-gradient": True})
    q["topology"] = {"name": "ring"}
    assert not train.sample_run(q)
    with pytest.raises(ValueError, match=r"--device-training: --clique-gradient"):
        train.check_eligible(_nodes(q), q, {"edges": {}})
    # the other refusals still apply
    monkeypatch.setenv("NIIDMIX_DEVICES", "0,1")
    with pytest.raises(ValueError, match="--device-training-sample runs on one device"):
        train.check_eligible(_nodes(p), p, _topo())
    monkeypatch.delenv("NIIDMIX_DEVICES")
    nodes = _nodes(p)
    nodes[2]["optimizer"] = torch.optim.SGD(nodes[2]["model"].parameters(), lr=0.5)
    with pytest.raises(ValueError, match="--device-training-sample needs the plugin's SGD"):
        train.check_eligible(nodes, p, _topo())
    q = _params()
    q["topology"]["sample-size"] = 7
    with pytest.raises(ValueError, match="--device-training-sample: sample-size 7"):
        train.check_eligible(_nodes(q), q, _topo())


def test_gn_lenet_sample_needs_both_keys():
    from niidmix import d_sgd, train
    two = lambda: [th.GNLeNet(), th.GNLeNet()]  # noqa: E731

    def nodes(p):
        out = th._nodes(p, two())
        for nd in out:
            nd["train-set"] = [(torch.zeros(1, 28, 28), 0)] * 4
        return out

    p = _params(**{GN: True, "batch-size": 4, "device-evaluation": False})
    p["topology"]["sample-size"] = 2
    assert train.check_eligible(nodes(p), p, _topo()) == (1, 10, 256)
    d_sgd.init(nodes(p), _topo(), p)
    q = _params(**{"batch-size": 4})
    q["topology"]["sample-size"] = 2
    with pytest.raises(ValueError, match=r"--device-training-sample trains linear models only.*gn-lenet"):
        train.check_eligible(nodes(q), q, _topo())


def _cpu_rounds(monkeypatch):
    """The CPU-path plugin over ROUNDS sample rounds, its device average stubbed out."""
    from niidmix import d_sgd
    monkeypatch.setattr(d_sgd, "_sample_cache", {})
    monkeypatch.setattr(d_sgd, "sample_average", lambda all_nodes, active: None)
    params = _params()
    del params["algorithm"]["device-training"], params["algorithm"][SAMPLE]
    torch.manual_seed(1234)
    nodes = _nodes(params)
    state, _, _ = d_sgd.init(nodes, _topo(), params)
    out = []
    for _ in range(ROUNDS):
        for n in nodes:
            n["model"].seen = []
        state, losses, done, active = d_sgd.next_step(state, params, None)
        out.append(([n["rank"] for n in active], [n["model"].seen[0] for n in active], done,
                    [n["epoch"] for n in nodes], sorted(losses)))
    return out, torch.get_rng_state()


def test_sample_rounds_draw_the_cpu_paths_batches(monkeypatch):
    """6 nodes of 50 samples, batch 16, random-with-overlap 3 / 1, 9 rounds (they cross an epoch):
    get_sample + train.draw on the active list give the CPU path's active ranks, samples,
    epoch_done, node['epoch'] and final RNG state; inactive nodes' iterators are untouched."""
    from niidmix import d_sgd, train
    cpu, rng_cpu = _cpu_rounds(monkeypatch)
    assert any(any(d.values()) for _, _, d, _, _ in cpu)             # an epoch ended on the way

    monkeypatch.setattr(d_sgd, "_sample_cache", {})
    params = _params()
    torch.manual_seed(1234)
    nodes = _nodes(params)
    state, _, _ = d_sgd.init(nodes, _topo(), params)
    for k in range(ROUNDS):
        active = d_sgd.get_sample(state, params, k)
        idle = {n["rank"]: n["train-iterator"] for n in nodes if all(n is not a for a in active)}
        batches, done = train.draw(active, params)
        ranks = [n["rank"] for n in active]
        markers = [[float(1000 * n["rank"] + j) for j in idx.tolist()] for n, idx in zip(active, batches)]
        assert ranks == cpu[k][0] and sorted(ranks) == cpu[k][4], f"round {k}"
        assert markers == cpu[k][1], f"round {k}"
        assert done == cpu[k][2] and [n["epoch"] for n in nodes] == cpu[k][3], f"round {k}"
        assert len(idle) == 3 and all(nodes[r]["train-iterator"] is it for r, it in idle.items())
    assert torch.equal(torch.get_rng_state(), rng_cpu)


def test_first_flag_is_set_in_the_first_round_that_samples_a_row(monkeypatch):
    from niidmix import d_sgd, train
    monkeypatch.setattr(d_sgd, "_sample_cache", {})
    params = _params()
    nodes = _nodes(params)
    state = {"nodes": nodes, "step": 0}
    stepped, first_round, seen = set(), {}, []
    for k in range(ROUNDS):
        rows = [n["rank"] for n in d_sgd.get_sample(state, params, k)]
        flags = train.first_flags(stepped, rows)
        assert len(flags) == len(rows) == 3
        for r, f in zip(rows, flags):
            assert f in (0, 1)
            if f:
                assert r not in first_round
                first_round[r] = k
            seen.append((k, r, f))
    for k, r, f in seen:
        assert f == int(first_round[r] == k), (k, r)
    assert stepped == set(first_round) and len(first_round) > 3      # later rounds bring new rows
    assert any(f == 0 for _, _, f in seen)                           # and sample old ones again


def test_sample_step_argument_errors_without_gpu():
    """Validation happens before any HIP call, so the documented codes come back on a CPU-only
    host too (the made-up addresses are never dereferenced)."""
    from niidmix import _lib
    L = _lib.lib
    F = L.niidmix_sample_step_mean_update_f32
    n, k, p = 5, 3, 8
    X, Y, G, B = 1 << 20, 1 << 24, 1 << 28, 1 << 32

    def call(x=X, ld_x=p, y=Y, ld_y=p, g=G, ld_g=p, buf=B, ld_b=p, active=8, first=8, mom=0.9,
             ncols=p, n_rows=n, k=k):
        return F(x, ld_x, y, ld_y, g, ld_g, buf, ld_b, active, first, 1.0 / k if k else 0.0, -0.1, mom,
                 ncols, n_rows, k, None)

    def err():
        return L.niidmix_last_error()

    for name in ("x", "y", "g", "buf", "active", "first"):
        assert call(**{name: None}) == _lib.EINVAL and b"null" in err(), name
    assert call(buf=None, first=None, mom=0.0, ncols=0) == _lib.OK    # both optional without momentum
    for name in ("x", "y", "g", "active"):
        assert call(**{name: None}, mom=0.0) == _lib.EINVAL, name
    assert call(k=0) == _lib.EINVAL and b"k 0" in err()
    assert call(k=n + 1) == _lib.EINVAL
    assert call(k=-1) == _lib.EINVAL and b"negative" in err()
    assert call(ncols=-1) == _lib.EINVAL and call(n_rows=-1) == _lib.EINVAL
    for name in ("ld_x", "ld_y", "ld_g", "ld_b"):
        assert call(**{name: p - 1}) == _lib.EINVAL and b"leading dimension" in err(), name
    assert call(y=X) == _lib.EALIAS and b"x and y" in err()
    assert call(y=X + 4 * ((n - 1) * p + p - 1)) == _lib.EALIAS      # y starts at x's last element
    assert call(g=Y + 4 * p) == _lib.EALIAS and b"g and y" in err()
    assert call(buf=Y) == _lib.EALIAS and call(buf=X) == _lib.EALIAS and call(buf=G) == _lib.EALIAS
    # g and buf span k rows at least: the last element of g's k-th row
    assert call(buf=G + 4 * ((k - 1) * p + p - 1)) == _lib.EALIAS


def test_header_and_op_declare_the_new_entry():
    from niidmix import _lib
    text = open(os.path.join(REPO, "include", "niidmix.h")).read()
    assert re.search(r"^int niidmix_sample_step_mean_update_f32\(", text, re.M)
    assert "#define NIIDMIX_ABI_VERSION 6" in text and _lib.lib.niidmix_abi_version() == 6
    assert "niidmix_sample_step_mean_update_f32" in _lib.SIGNATURES
    from niidmix import ops
    assert hasattr(torch.ops.niidmix, "sample_step_mean_update") and callable(ops.sample_step_mean_update)
