"""--device-sampling on the GPU: niidmix::draw_batches against the host restatement
(niidmix.sampling), exact equality; the launcher's refusals through the C-ABI; and whole rounds
through d_sgd.init / next_step, which equal, bit for bit, the same trainer's existing rounds fed
the restatement's index tensors (the kernels and the indices are the same, so the bits are)."""
import numpy as np
import pytest
import torch

import test_gpu_train as tg
import test_gpu_train_sample as tgs

pytestmark = pytest.mark.gpu

SEED = 2027
_perms = {}


def _perm(rank, epoch, length):
    """The restatement's permutation, computed once per (rank, epoch, length)."""
    from niidmix.sampling import epoch_permutation
    key = (rank, epoch, length)
    if key not in _perms:
        _perms[key] = epoch_permutation(SEED, rank, epoch, length)
    return _perms[key]


def _jobs(b_max, most):
    """(rank, seg_start, seg_len, epoch, cursor) per job: every length at which the kernel takes
    another path (one wave up to 64; the powers of two and their neighbours of the padded network;
    the LDS limit), each with a cursor at 0, in the middle and on the last (short) batch, in epochs
    0, 1 and 2^31 - 1; ranks out of order, segment starts repeated."""
    jobs = []
    for length in (1, 2, 3, 63, 64, 65, 600, 1023, 1024, 1025, most - 1, most):
        cursors = (0, length // 2, (length - 1) // b_max * b_max)
        for cursor, epoch in zip(cursors, (0, 1, 2 ** 31 - 1)):
            j = len(jobs)
            jobs.append(((7 * j + 3) % 11, (j % 3) * 20000, length, epoch, cursor))
        jobs.append((5, 0, length, 1, 0))                    # another epoch at the same cursor
    return jobs


@pytest.mark.parametrize("b_max", [1, 16, 125])
def test_op_equals_the_host_restatement(gpu, b_max):
    from niidmix import ops
    most = ops.draw_batches_max_len()
    jobs = _jobs(b_max, most)
    cols = [torch.tensor(c, dtype=torch.int32, device=gpu) for c in zip(*jobs)]
    n = len(jobs)
    bi = torch.full((n, b_max), -7, dtype=torch.int32, device=gpu)
    bl = torch.full((n,), -7, dtype=torch.int32, device=gpu)
    torch.ops.niidmix.draw_batches(SEED, *cols, bi, bl)
    got_i, got_l = bi.cpu().numpy(), bl.cpu().numpy()
    short = 0
    for j, (rank, start, length, epoch, cursor) in enumerate(jobs):
        want = start + _perm(rank, epoch, length)[cursor:cursor + b_max]
        assert got_l[j] == len(want) == min(b_max, length - cursor), (j, jobs[j])
        assert np.array_equal(got_i[j, :len(want)], want), (j, jobs[j])
        assert (got_i[j, len(want):] == -7).all(), (j, jobs[j])      # the sentinel stays
        short += len(want) < b_max
    assert short or b_max == 1                                         # len < b_max occurred
    bi2, bl2 = torch.full_like(bi, -7), torch.full_like(bl, -7)
    torch.ops.niidmix.draw_batches(SEED, *cols, bi2, bl2)
    assert torch.equal(bi2, bi) and torch.equal(bl2, bl)               # two calls, the same bits
    # the seed is part of the key
    torch.ops.niidmix.draw_batches(SEED + 1, *cols, bi2, bl2)
    assert torch.equal(bl2, bl) and not torch.equal(bi2, bi)


def test_op_refuses_wrong_tensors(gpu):
    from niidmix import ops
    v = lambda: torch.zeros(3, dtype=torch.int32, device=gpu)          # noqa: E731
    bi = torch.zeros(3, 4, dtype=torch.int32, device=gpu)
    ok = [v(), v(), v(), v(), v(), bi, v()]
    for pos, bad in ((1, v().long()), (2, v().cpu()), (3, torch.zeros(4, dtype=torch.int32, device=gpu)),
                     (6, bi.t().contiguous().t()), (6, bi.float()), (7, ok[1]), (7, v()[:2]),
                     (6, torch.zeros(3, ops.draw_batches_max_len() + 1, dtype=torch.int32, device=gpu))):
        args = list(ok)
        args[pos - 1] = bad
        with pytest.raises(RuntimeError):
            torch.ops.niidmix.draw_batches(SEED, *args)


def test_launcher_refusals_through_the_c_abi(gpu):
    """Each is refused before any launch: the outputs keep their fill."""
    from niidmix import _lib
    L = _lib.lib
    n, b = 4, 8
    ins = [torch.ones(n, dtype=torch.int32, device=gpu) for _ in range(5)]
    bi = torch.full((n, b), -7, dtype=torch.int32, device=gpu)
    bl = torch.full((n,), -7, dtype=torch.int32, device=gpu)

    def call(n_jobs=n, b_max=b, ptrs=None):
        p = [t.data_ptr() for t in ins + [bi, bl]] if ptrs is None else ptrs
        return L.niidmix_draw_batches_i32(SEED, *p[:5], n_jobs, b_max, p[5], p[6], None)

    base = [t.data_ptr() for t in ins + [bi, bl]]
    for k in range(7):
        assert call(ptrs=base[:k] + [None] + base[k + 1:]) == _lib.EINVAL
        assert b"null" in L.niidmix_last_error()
    assert call(n_jobs=0) == _lib.EINVAL and call(b_max=0) == _lib.EINVAL
    assert call(b_max=L.niidmix_draw_batches_max_len() + 1) == _lib.EUNSUPPORTED
    assert call(ptrs=base[:6] + [base[0]]) == _lib.EALIAS             # batch_len on rank
    assert call(ptrs=base[:4] + [base[5] + 4 * (n * b - 1)] + base[5:]) == _lib.EALIAS   # cursor in batch_idx
    assert call(ptrs=base[:6] + [base[5] + 4]) == _lib.EALIAS         # the outputs on each other
    torch.cuda.synchronize()
    assert bool((bi == -7).all()) and bool((bl == -7).all())


# ------------------------------------------------------------------------------------------------
# whole rounds
class _Ring:
    def __init__(self, n):
        w = torch.zeros(n, n)
        for i in range(n):
            for j in (i - 1, i, i + 1):
                w[i, j % n] = 1.0 / 3.0
        self.topo = {"edges": {i: [(i - 1) % n, (i + 1) % n] for i in range(n)}, "weights": w}


#         model, sample shape, classes, nodes, samples per node, batch, rounds, lr, flags, topology
CASES = {
    "linear": (tg.Net, (1, 28, 28), 10, 16, 60, 25, 5, 0.1, ("device-training",), "ring"),
    "sample": (tgs.Linear, (33,), 7, 16, 7, 4, 3, 0.1, ("device-training", "device-training-sample"),
               "sample"),
    "gn-lenet": (tgs.GN, (1, 15, 15), 3, 4, 4, 2, 2, 0.05, ("device-training", "device-training-gn-lenet"),
                 "ring"),
}
_data = {}


def _dataset(case):
    if case not in _data:
        _, shape, c, n, s = CASES[case][:5]
        g = torch.Generator().manual_seed(77)
        # sparse, bounded inputs: SGD at lr 0.1 is stable on them
        lit = 0.05 if case == "linear" else 0.3
        x = torch.rand(n * s, *shape, generator=g) * (torch.rand(n * s, *shape, generator=g) < lit)
        if case == "gn-lenet":
            x = torch.randn(n * s, *shape, generator=g)
        _data[case] = (x, torch.randint(0, c, (n * s,), generator=g))
    return _data[case]


def _restated_loader(node, params):
    """train.index_loader's stand-in for the run without the flag: the epoch's batches of the host
    restatement, as int64 index tensors (what the existing round packs and uploads)."""
    length, b = len(node["train-set"]), int(params["algorithm"]["batch-size"])
    perm = _perm(node["rank"], node["epoch"], length)
    return iter([torch.from_numpy(perm[c:c + b].copy()) for c in range(0, length, b)])


def _run(case, sampling, momentum, monkeypatch):
    """The plugin's rounds, on the device's own sampling (`sampling`) or on the existing round fed
    the restatement's batches.  Returns the per-round log and the trainer."""
    from niidmix import d_sgd, train
    from niidmix.sampling import SamplerState
    model, _, _, n, s, batch, rounds, lr, flags, topology = CASES[case]
    monkeypatch.setattr(d_sgd, "_sample_cache", {})
    if not sampling:
        monkeypatch.setattr(train, "index_loader", _restated_loader)
    params = {"meta": {"log": "WARNING", "seed": SEED}, "nodes": {"nb-nodes": n},
              "topology": {"name": "sample", "sample-method": "random-with-overlap", "sample-size": 4,
                           "sample-overlap": 1} if topology == "sample" else
              {"name": "ring", "remove-clique-edges": 0},
              "logger": {"accuracy-logging-interval": 0, "accuracy-logging-interval-steps": 0,
                         "log-consensus-distance": False},
              "algorithm": {"learning-rate": lr, "learning-momentum": momentum, "batch-size": batch,
                            "initial-averaging": False, "clique-gradient": False,
                            "unbiased-gradient": False, "deferred-writeback": False,
                            "mixing-mode": "exact", **{f: True for f in flags},
                            **({"device-sampling": True} if sampling else {})}}
    x, y = _dataset(case)
    torch.manual_seed(2028)
    gen = torch.Generator().manual_seed(2029)
    nodes = []
    for r in range(n):
        mdl = model()
        if case == "gn-lenet":
            tgs.th.perturb(mdl, gen)
        nodes.append({"rank": r, "epoch": 0, "model": mdl, "optimizer": d_sgd.optimizer(mdl, params),
                      "train-set": [(x[r * s + j], int(y[r * s + j])) for j in range(s)]})
    topo = {"edges": {}, "weights": []} if topology == "sample" else _Ring(n).topo
    state, _, _ = d_sgd.init(nodes, topo, params)
    assert all((nd["train-iterator"] is None) == sampling for nd in nodes)
    st = SamplerState(range(n), [s] * n, batch)
    log, tr = [], None
    for k in range(rounds):
        state, losses, done, active = d_sgd.next_step(state, params, None)
        d_sgd.synchronize()
        rows = [nd["rank"] for nd in active]
        epoch, cursor, want_done = st.advance(rows)
        assert done == want_done and [nd["epoch"] for nd in nodes] == st.epoch.tolist(), f"round {k}"
        assert sorted(losses) == sorted(rows) and all(np.isfinite(v) for v in losses.values())
        tr = d_sgd._trainers[id(nodes)]
        assert tr.sampling == sampling
        # the index block the gradient op read: the restatement's batches, node offsets added
        bi = tr.layout.view(tr.idx_dev, "indices").cpu().numpy()
        bl = tr.layout.view(tr.idx_dev, "lengths").cpu().numpy()
        for j, (r, e, c) in enumerate(zip(rows, epoch.tolist(), cursor.tolist())):
            want = r * s + _perm(r, e, s)[c:c + batch]
            assert bl[j] == len(want) and np.array_equal(bi[j, :len(want)], want), (k, j)
        log.append((rows, losses, done, tgs._flat(nodes)))
    assert any(any(d.values()) for _, _, d, _ in log)                 # an epoch ended on the way
    return log, tr


@pytest.mark.parametrize("case,momentum", [("linear", 0.0), ("linear", 0.9), ("sample", 0.0),
                                           ("sample", 0.9), ("gn-lenet", 0.9)])
def test_rounds_equal_the_existing_round_on_the_same_indices(gpu, monkeypatch, case, momentum):
    log_s, tr = _run(case, True, momentum, monkeypatch)
    assert tr.sample == (case == "sample") and tr.kind == ("gn-lenet" if case == "gn-lenet" else "linear")
    log_h, _ = _run(case, False, momentum, monkeypatch)
    assert len(log_s) == len(log_h) == CASES[case][6]
    for k, ((rows_s, loss_s, done_s, th_s), (rows_h, loss_h, done_h, th_h)) in enumerate(zip(log_s, log_h)):
        assert rows_s == rows_h and done_s == done_h, f"round {k}"
        assert loss_s == loss_h, f"round {k}"                         # the same floats
        assert torch.equal(th_s.view(torch.int32), th_h.view(torch.int32)), f"round {k}"
    assert not torch.equal(log_s[0][3], log_s[-1][3])                 # and the models moved


def test_sampling_consumes_no_torch_rng(gpu, monkeypatch):
    """Rounds under the flag leave the global torch RNG where the models' initialisation left it."""
    from niidmix import d_sgd
    seen = []
    orig = d_sgd.init

    def init(nodes, topo, params):
        out = orig(nodes, topo, params)
        seen.append(torch.get_rng_state())
        return out
    monkeypatch.setattr(d_sgd, "init", init)
    _run("sample", True, 0.0, monkeypatch)
    assert len(seen) == 1 and torch.equal(torch.get_rng_state(), seen[0])
