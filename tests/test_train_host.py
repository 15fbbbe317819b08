"""--device-training, the parts that need no GPU: the index loaders draw the CPU path's samples
from the CPU path's RNG stream, the refusals, the C entry point's argument checks, the header."""
import os
import re

import pytest
import torch

from conftest import REPO


class Net(torch.nn.Module):
    def __init__(self, k=6, c=3):
        super().__init__()
        self.fc = torch.nn.Linear(k, c)

    def forward(self, x, params):
        return torch.nn.functional.log_softmax(self.fc(x.view(-1, self.fc.in_features)), dim=1)


class Net3(Net):
    def __init__(self):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.ones(1))


def _params(**alg):
    a = {"learning-rate": 0.1, "learning-momentum": 0.0, "batch-size": 16, "initial-averaging": False,
         "clique-gradient": False, "unbiased-gradient": False, "device-training": True}
    a.update(alg)
    return {"meta": {"log": "WARNING"}, "topology": {"name": "ring"}, "algorithm": a,
            "logger": {}}


def _nodes(params, n=2, samples=50, model=Net):
    from niidmix import d_sgd
    nodes = []
    for r in range(n):
        # sample j of node r carries the marker value 1000 r + j in every feature
        ts = [(torch.full((6,), float(1000 * r + j)), j % 3) for j in range(samples)]
        mdl = model()
        nodes.append({"rank": r, "epoch": 0, "train-set": ts, "model": mdl,
                      "optimizer": d_sgd.optimizer(mdl, params)})
    return nodes


def test_index_loader_draws_the_cpu_paths_samples():
    """50 samples, batch 16, two epochs plus one step (9 rounds): the trainer's loaders yield the
    indices of exactly the samples the CPU path's loaders yield (identified by their marker), and
    leave the global RNG, epoch_done and node['epoch'] as the CPU path does."""
    from niidmix import d_sgd, train
    params = _params()
    rounds = 2 * 4 + 1

    torch.manual_seed(1234)
    nodes = _nodes(params)
    for n in nodes:                                          # d_sgd.init
        n["train-iterator"] = d_sgd._loader(n, params)
    cpu = []
    for _ in range(rounds):                                  # d_sgd.next_step's sampling
        markers, done = [], {}
        for n in nodes:
            data, _ = next(n["train-iterator"])
            markers.append(data[:, 0].tolist())
            rest = d_sgd._peek(n["train-iterator"])
            done[n["rank"]] = rest is None
            if rest is None:
                n["epoch"] += 1
                n["train-iterator"] = d_sgd._loader(n, params)
            else:
                n["train-iterator"] = rest
        cpu.append((markers, done, [n["epoch"] for n in nodes]))
    rng_cpu = torch.get_rng_state()

    torch.manual_seed(1234)
    nodes = _nodes(params)
    for n in nodes:
        n["train-iterator"] = train.index_loader(n, params)
    for k in range(rounds):
        batches, done = train.draw(nodes, params)
        markers = [[float(1000 * n["rank"] + j) for j in idx.tolist()] for n, idx in zip(nodes, batches)]
        assert markers == cpu[k][0], f"round {k}"
        assert done == cpu[k][1] and [n["epoch"] for n in nodes] == cpu[k][2], f"round {k}"
    assert torch.equal(torch.get_rng_state(), rng_cpu)
    assert [n["epoch"] for n in nodes] == [2, 2]
    assert [len(m) for m in cpu[3][0]] == [2, 2]             # an epoch's last batch is short


def test_refusals_name_the_flag():
    from niidmix import d_sgd
    p = _params()
    with pytest.raises(ValueError, match="device-training"):
        d_sgd.init(_nodes(p, model=Net3), {"edges": {}}, p)
    p = _params()
    p["topology"]["name"] = "sample"
    with pytest.raises(ValueError, match="device-training"):
        d_sgd.init(_nodes(p), {"edges": {}}, p)
    p = _params(**{"clique-gradient": True})
    with pytest.raises(ValueError, match="device-training"):
        d_sgd.init(_nodes(p), {"edges": {}}, p)
    p = _params(**{"unbiased-gradient": True})
    with pytest.raises(ValueError, match="device-training"):
        d_sgd.init(_nodes(p), {"edges": {}}, p)


def test_cli_flag_is_a_store_const(tmp_path, monkeypatch):
    """--device-training writes params['algorithm']['device-training'] = True and is absent by
    default."""
    import json
    from niidmix import d_sgd
    for argv, want in (([], None), (["--device-training"], True)):
        run = tmp_path / ("on" if want else "off")
        run.mkdir()
        (run / "params.json").write_text(json.dumps({"topology": {"name": "ring"}}))
        monkeypatch.setattr(d_sgd, "load_topology", lambda rundir: {"edges": {}})
        d_sgd.main(["--rundir", str(run)] + argv)
        alg = json.loads((run / "params.json").read_text())["algorithm"]
        assert alg.get("device-training") is want


def test_grad_argument_errors_without_gpu():
    """Validation happens before any HIP call, so the documented codes come back on a CPU-only
    host too (the made-up addresses are never dereferenced)."""
    from niidmix import _lib
    L = _lib.lib
    F = L.niidmix_linear_nll_grad_rows_f32
    E = L.niidmix_linear_nll_grad_rows_scratch_elems
    base, far, scr = 1 << 20, 1 << 30, 1 << 40
    k, c, b = 5, 3, 4
    p = c * k + c

    def call(theta=base, ld_t=p, data=8, labels=8, bidx=8, blen=8, b_max=b, rows=8, n_rows=2,
             grad=far, ld_g=p, loss=8, K=k, C=c, scratch=scr, elems=None):
        if elems is None:
            elems = E(n_rows, b_max, C)
        return F(theta, ld_t, data, labels, bidx, blen, b_max, rows, n_rows, grad, ld_g, loss, K, C,
                 scratch, elems, None)

    def err():
        return L.niidmix_last_error()

    assert E(2, 4, 3) >= 2 * 4 * 3 and E(0, 4, 3) == 0
    for name in ("theta", "data", "labels", "bidx", "blen", "rows", "grad", "loss", "scratch"):
        assert call(**{name: None}) == _lib.EINVAL and b"null" in err(), name
    assert call(n_rows=-1, elems=0) == _lib.EINVAL and b"negative" in err()
    assert call(n_rows=0, theta=None) == _lib.OK                                  # empty before null
    assert call(ld_t=p - 1) == _lib.EINVAL and b"leading dimension < C * K + C" in err()
    assert call(ld_g=p - 1) == _lib.EINVAL
    assert call(elems=1) == _lib.EINVAL and b"scratch" in err()
    assert call(grad=base) == _lib.EALIAS and b"theta and grad" in err()
    assert call(grad=base + 4 * (p + 2)) == _lib.EALIAS      # grad starts inside theta's 2nd row
    assert call(b_max=32768 // 3 + 1) == _lib.EUNSUPPORTED and b"b_max * C" in err()
    assert call(C=1025, ld_t=1025 * k + 1025, ld_g=1025 * k + 1025, b_max=1) == _lib.EUNSUPPORTED
    assert call(ld_t=p - 1, b_max=32768) == _lib.EUNSUPPORTED                      # limits before ld


def test_header_declares_the_new_symbol_at_abi_6():
    from niidmix import _lib
    assert _lib.lib.niidmix_abi_version() == 6
    text = open(os.path.join(REPO, "include", "niidmix.h")).read()
    assert re.search(r"^int niidmix_linear_nll_grad_rows_f32\(", text, re.M)
    assert re.search(r"^int64_t niidmix_linear_nll_grad_rows_scratch_elems\(", text, re.M)
    assert "#define NIIDMIX_ABI_VERSION 6" in text
    assert "niidmix_linear_nll_grad_rows_f32" in _lib.SIGNATURES
