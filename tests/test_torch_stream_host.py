"""--device-sampling-torch-stream, the parts that need no GPU: the host model of torch's stream
(niidmix.sampling: torch_permutation against torch.randperm, LoaderDraws against real index
loaders under train.draw), the flag, its CLI keys and its refusals.  Every comparison is exact."""
import json

import numpy as np
import pytest
import torch

import test_train_sample_host as tsh

KEY = "device-sampling-torch-stream"
LENGTHS, BATCH, ROUNDS = [5, 7, 4, 10, 3], 3, 9


@pytest.mark.parametrize("n", [1, 2, 3, 64, 625, 1249, 8193, 60000])
def test_torch_permutation_equals_torch_randperm(n):
    from niidmix.sampling import torch_permutation
    g = torch.Generator()
    for seed in (0, 1, 5489, 2 ** 31, 2 ** 32 - 1, 2 ** 32 + 7, 2 ** 63 - 5):
        g.manual_seed(seed)
        want = torch.randperm(n, generator=g).numpy()
        got = torch_permutation(seed, n)
        assert got.dtype == np.int64 and np.array_equal(got, want), (n, seed)
        if seed == 2 ** 32 + 7:          # only the low 32 bits count
            assert np.array_equal(got, torch_permutation(7, n))


def test_one_vectorised_draw_equals_scalar_draws():
    torch.manual_seed(91)
    scalar = [int(torch.empty((), dtype=torch.int64).random_().item()) for _ in range(2000)]
    after_scalar = torch.get_rng_state()
    torch.manual_seed(91)
    vector = torch.empty(2000, dtype=torch.int64).random_().tolist()
    assert vector == scalar and torch.equal(torch.get_rng_state(), after_scalar)
    assert len(set(scalar)) == 2000 and max(scalar) >= 2 ** 32


def _loader_rounds(samples):
    """train.draw on real index loaders: per round the batches, epoch_done, every node's epoch and
    the global generator's state."""
    from niidmix import train
    params = {"algorithm": {"batch-size": BATCH}}
    torch.manual_seed(77)
    nodes = [{"rank": r, "epoch": 0, "train-set": list(range(n))} for r, n in enumerate(LENGTHS)]
    for nd in nodes:
        nd["train-iterator"] = train.index_loader(nd, params)
    out = []
    for rows in samples:
        batches, done = train.draw([nodes[r] for r in rows], params)
        out.append(([b.tolist() for b in batches], done, [nd["epoch"] for nd in nodes], torch.get_rng_state()))
    return out


def _model_rounds(samples):
    """The same from LoaderDraws, torch_permutation and a SamplerState: no loader."""
    from niidmix.sampling import LoaderDraws, SamplerState, torch_permutation
    torch.manual_seed(77)
    st = SamplerState(range(len(LENGTHS)), LENGTHS, BATCH)
    LoaderDraws.at_init(len(LENGTHS))
    perms, out = {}, []
    for rows in samples:
        rows = np.asarray(rows)
        begins = st.cached[rows] != st.epoch[rows]
        assert np.array_equal(rows[begins], st.stale(rows))
        seeds = LoaderDraws.round(begins, st.cursor[rows] + BATCH >= st.length[rows])
        assert seeds.shape == (int(begins.sum()),) and ((0 <= seeds) & (seeds < 2 ** 32)).all()
        for r, s in zip(rows[begins].tolist(), seeds.tolist()):
            perms[r] = torch_permutation(s, LENGTHS[r])
        st.mark_cached(rows[begins])
        _, cursor, done = st.advance(rows)
        batches = [perms[r][c:c + BATCH].tolist() for r, c in zip(rows.tolist(), cursor.tolist())]
        out.append((batches, done, st.epoch.tolist(), torch.get_rng_state()))
    return out


@pytest.mark.parametrize("samples", [
    [list(range(5))] * ROUNDS,
    # two of five rows a round, in the sample's order: rows advance at different rates
    [[2, 0], [1, 3], [0, 4], [4, 2], [3, 1], [0, 2], [2, 4], [1, 0], [3, 4]],
], ids=["graph", "sample"])
def test_loader_draws_equal_train_draw_on_real_loaders(samples):
    want, got = _loader_rounds(samples), _model_rounds(samples)
    assert len(want) == len(got) == ROUNDS
    for k, (w, g) in enumerate(zip(want, got)):
        assert g[0] == w[0], f"round {k}: batches"
        assert g[1] == w[1] and g[2] == w[2], f"round {k}: epoch_done / epochs"
        assert torch.equal(g[3], w[3]), f"round {k}: RNG state"
    assert any(any(w[1].values()) for w in want) and max(want[-1][2]) >= 2


def _params(**alg):
    return tsh._params(**{"device-sampling": True, KEY: True, **alg})


def test_flag_is_accepted_without_a_seed_and_bounded_by_the_kernel():
    from niidmix import ops, train
    most = ops.torch_randperm_max_len()
    assert most == 65536
    p = _params()
    assert "seed" not in p["meta"]
    assert train.torch_stream_enabled(p) and train.cached_enabled(p) and train.sampling_enabled(p)
    nodes = tsh._nodes(p)
    assert train.check_eligible(nodes, p, tsh._topo()) == (6, 3)
    nodes[3]["train-set"] = range(most)          # a range stands in for the samples: only len() is read
    assert train.check_eligible(nodes, p, tsh._topo()) == (6, 3)
    nodes[3]["train-set"] = range(most + 1)
    with pytest.raises(ValueError, match=rf"--{KEY}: node 3's train-set has {most + 1} samples"):
        train.check_eligible(nodes, p, tsh._topo())
    # the batch: the kernels' ordinary limit, and the shuffle's under --device-training-large-batch
    q = _params(**{"device-training-large-batch": True, "batch-size": most})
    assert train.check_eligible(tsh._nodes(q), q, tsh._topo()) == (6, 3)
    q = _params(**{"device-training-large-batch": True, "batch-size": most + 1})
    with pytest.raises(ValueError, match=rf"--{KEY}: batch size {most + 1} is not in 1..{most}"):
        train.check_eligible(tsh._nodes(q), q, tsh._topo())
    # without the flag nothing changes: the seed is asked for
    q = tsh._params(**{"device-sampling": True})
    with pytest.raises(ValueError, match="--device-sampling .*seed"):
        train.check_eligible(tsh._nodes(q), q, tsh._topo())


def test_flag_needs_device_sampling():
    from niidmix import d_sgd, train
    q = _params()
    del q["algorithm"]["device-sampling"]
    for call in (lambda: train.check_eligible(tsh._nodes(q), q, tsh._topo()),
                 lambda: d_sgd.init(tsh._nodes(q), tsh._topo(), q)):
        with pytest.raises(ValueError, match=f"--{KEY} .*needs --device-sampling"):
            call()
    del q["algorithm"]["device-training"], q["algorithm"][tsh.SAMPLE]
    with pytest.raises(ValueError, match=f"--{KEY} .*needs --device-sampling"):
        d_sgd.init(tsh._nodes(q), tsh._topo(), q)


def test_init_draws_the_loaders_base_seeds_and_builds_no_loader():
    from niidmix import d_sgd
    p = _params()
    torch.manual_seed(5)
    nodes = tsh._nodes(p)
    after_nodes = torch.get_rng_state()
    state, _, _ = d_sgd.init(nodes, tsh._topo(), p)
    assert all(n["train-iterator"] is None for n in state["nodes"])
    flagged = torch.get_rng_state()
    # the CPU path's init, from the same state: loaders, and the generator in the same place
    q = tsh._params()
    torch.manual_seed(5)
    nodes = tsh._nodes(q)
    assert torch.equal(torch.get_rng_state(), after_nodes)
    state, _, _ = d_sgd.init(nodes, tsh._topo(), q)
    assert all(n["train-iterator"] is not None for n in state["nodes"])
    assert torch.equal(torch.get_rng_state(), flagged) and not torch.equal(flagged, after_nodes)


class _Trainer:
    """What d_sgd's switched-flag loop reads of a live trainer."""
    sample, sampling, cached, large, mom_steps = True, True, True, False, 0

    def __init__(self, torch_stream):
        self.torch_stream = torch_stream

    def owns(self, nodes):
        return True


@pytest.mark.parametrize("built_with", [False, True])
def test_a_switch_of_the_flag_during_the_run_is_refused(monkeypatch, built_with):
    from niidmix import d_sgd
    p = _params() if not built_with else tsh._params(**{"device-sampling": True, "device-sampling-cached": True})
    nodes = tsh._nodes(p)
    monkeypatch.setattr(d_sgd, "_trainers", {id(nodes): _Trainer(built_with)})
    state = {"nodes": nodes, "topology": tsh._topo(), "step": 0}
    with pytest.raises(ValueError, match=f"--{KEY} was switched during the run"):
        d_sgd.next_step(state, p, None)


def test_cli_flag_writes_its_keys_and_needs_device_sampling(tmp_path, monkeypatch, capsys):
    from niidmix import d_sgd
    monkeypatch.setattr(d_sgd, "load_topology", lambda rundir: tsh._topo())
    run = tmp_path / "run"
    run.mkdir()
    (run / "params.json").write_text(json.dumps({"topology": {"name": "sample"}}))
    d_sgd.main(["--rundir", str(run), "--device-training", "--device-sampling", f"--{KEY}"])
    alg = json.loads((run / "params.json").read_text())["algorithm"]
    assert (alg.get("device-sampling"), alg.get("device-sampling-cached"), alg.get(KEY)) == (True, True, True)
    run = tmp_path / "alone"
    run.mkdir()
    (run / "params.json").write_text(json.dumps({"topology": {"name": "ring"}}))
    with pytest.raises(SystemExit):
        d_sgd.main(["--rundir", str(run), "--device-training", f"--{KEY}"])
    assert f"--{KEY} needs --device-sampling" in capsys.readouterr().err
    assert "algorithm" not in json.loads((run / "params.json").read_text())


def test_source_class_keeps_its_callers_and_gains_the_mode():
    from niidmix import batches
    assert batches.source_class(False, True, True) is batches.CachedSource
    assert batches.source_class(False, True, True, True) is batches.TorchStreamSource
    assert batches.source_class(True, False, False, True) is batches.LoaderSource
    assert issubclass(batches.TorchStreamSource, batches.CachedSource)
