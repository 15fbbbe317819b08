"""--device-sampling-cached on the GPU: niidmix::epoch_perm and niidmix::take_batches against the
host restatement (niidmix.sampling) and against niidmix::draw_batches, exact equality; the ops'
refusals; and whole rounds through d_sgd.init / next_step with train-sets on both sides of the 8192
samples one workgroup sorts, which equal, bit for bit, the same trainer's existing rounds fed the
restatement's index tensors."""
import numpy as np
import pytest
import torch

import test_gpu_sampling as tgsamp
import test_gpu_train_sample as tgs

pytestmark = pytest.mark.gpu

SEED = tgsamp.SEED
_perm = tgsamp._perm            # the restatement's permutation, computed once per (rank, epoch, length)
SHORT = (1, 64, 65, 8191, 8192)
LONG = (8193, 16384, 16385, 24577, 65536, 100003)
EPOCHS = (0, 1, 2 ** 31 - 2)
FILL = -7
_cache = {}


def _layout(lengths):
    """(rank, epoch, perm_off) per job and the cache's size: ranks out of order, the jobs' stretches
    in another order than the jobs, with gaps between, before and after them."""
    n = len(lengths)
    rank = [(7 * j + 3) % 11 for j in range(n)]
    epoch = [EPOCHS[j % 3] for j in range(n)]
    off, at = [0] * n, 5
    for j in sorted(range(n), key=lambda j: (3 * j + 1) % n):
        off[j] = at
        at += lengths[j] + 3 + j
    return rank, epoch, off, at + 11


def _sorted_cache(gpu, lengths, seed=SEED):
    """niidmix::epoch_perm over one call of the jobs `lengths`; the filled cache (device), computed
    once per job list and seed, and the jobs' columns."""
    from niidmix import ops
    key = (lengths, seed)
    if key not in _cache:
        rank, epoch, off, size = _layout(lengths)
        dev = lambda v, dt=torch.int32: torch.tensor(v, dtype=dt, device=gpu)   # noqa: E731
        perm = torch.full((size,), FILL, dtype=torch.int32, device=gpu)
        nbytes = ops.epoch_perm_scratch_bytes(len(lengths), max(lengths))
        scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=gpu)
        torch.ops.niidmix.epoch_perm(seed, dev(rank), dev(lengths), dev(epoch), dev(off, torch.int64),
                                     max(lengths), perm, scratch)
        _cache[key] = perm
    return _cache[key]


@pytest.mark.parametrize("lengths", [SHORT, LONG], ids=["short", "long"])
def test_epoch_perm_equals_the_host_restatement(gpu, lengths):
    from niidmix import ops
    assert (ops.epoch_perm_scratch_bytes(len(lengths), max(lengths)) == 0) == (lengths is SHORT)
    rank, epoch, off, size = _layout(lengths)
    got = _sorted_cache(gpu, lengths).cpu().numpy()
    untouched = np.ones(size, dtype=bool)
    for j, length in enumerate(lengths):
        want = _perm(rank[j], epoch[j], length)
        assert np.array_equal(got[off[j]:off[j] + length], want), (j, length)
        untouched[off[j]:off[j] + length] = False
    assert untouched.sum() > 2 * len(lengths) and (got[untouched] == FILL).all()    # the sentinel stays
    # two calls give the same bits, another seed gives others
    first = _cache.pop((lengths, SEED))
    assert torch.equal(_sorted_cache(gpu, lengths), first)
    assert not torch.equal(_sorted_cache(gpu, lengths, SEED + 1), first)


def test_epoch_perm_sorts_mixed_lengths_and_skips_what_does_not_fit(gpu):
    """One call may hold short and long jobs; a seg_len above max_len is clamped to it, a stretch
    that does not lie inside perm is skipped: nothing outside the jobs' stretches is written."""
    lengths = (70, 8193, 9000, 16385, 300, 20000)
    rank, epoch = [4, 1, 9, 0, 2, 5], [1, 0, 2, 1, 0, 0]
    size = 40000
    off = [0, 100, 9000, 18100, 39900, -5]                 # job 4 runs past the end, job 5 starts before it
    dev = lambda v, dt=torch.int32: torch.tensor(v, dtype=dt, device=gpu)   # noqa: E731
    perm = torch.full((size,), FILL, dtype=torch.int32, device=gpu)
    max_len = 16385
    from niidmix import ops
    scratch = torch.empty(ops.epoch_perm_scratch_bytes(6, max_len), dtype=torch.uint8, device=gpu)
    torch.ops.niidmix.epoch_perm(SEED, dev(rank), dev(lengths), dev(epoch), dev(off, torch.int64), max_len,
                                 perm, scratch)
    got = perm.cpu().numpy()
    untouched = np.ones(size, dtype=bool)
    for j in range(4):
        want = _perm(rank[j], epoch[j], lengths[j])
        assert np.array_equal(got[off[j]:off[j] + lengths[j]], want), j
        untouched[off[j]:off[j] + lengths[j]] = False
    assert (got[untouched] == FILL).all()
    # clamped: the permutation of the clamped length
    perm.fill_(FILL)
    torch.ops.niidmix.epoch_perm(SEED, dev(rank[:3]), dev(lengths[:3]), dev(epoch[:3]), dev(off[:3], torch.int64),
                                 8500, perm, scratch)
    got = perm.cpu().numpy()
    assert np.array_equal(got[9000:17500], _perm(rank[2], epoch[2], 8500)) and (got[17500:] == FILL).all()
    assert np.array_equal(got[100:8293], _perm(rank[1], epoch[1], 8193))


@pytest.mark.parametrize("b_max", [1, 16, 125])
def test_take_batches_equals_the_slice_and_draw_batches(gpu, b_max):
    lengths = SHORT + LONG
    rank, epoch, off, _ = _layout(SHORT)
    rank_l, epoch_l, off_l, size_l = _layout(LONG)
    short, long_ = _sorted_cache(gpu, SHORT), _sorted_cache(gpu, LONG)
    perm = torch.cat([long_, short])                       # one cache: the short jobs behind the long
    jobs = []                                              # (rank, seg_start, length, epoch, cursor, perm_off)
    for j, length in enumerate(lengths):
        r, e, o = (rank[j], epoch[j], off[j] + size_l) if j < len(SHORT) else \
            (rank_l[j - len(SHORT)], epoch_l[j - len(SHORT)], off_l[j - len(SHORT)])
        # cursor 0, in the middle and on the last (short) batch
        for cursor in (0, length // 2, (length - 1) // b_max * b_max):
            jobs.append((r, (len(jobs) % 3) * 20000, length, e, cursor, o))
    jobs += [(3, 0, 50, 0, 50, 5), (3, 0, 50, 0, -1, 5), (3, 0, 0, 0, 0, 5),       # empty batches
             (3, 0, 50, 0, 0, perm.numel() - 49)]
    n = len(jobs)
    col = lambda i, dt=torch.int32: torch.tensor([jb[i] for jb in jobs], dtype=dt, device=gpu)  # noqa: E731
    bi = torch.full((n, b_max), FILL, dtype=torch.int32, device=gpu)
    bl = torch.full((n,), FILL, dtype=torch.int32, device=gpu)
    torch.ops.niidmix.take_batches(perm, col(5, torch.int64), col(1), col(2), col(4), bi, bl)
    got_i, got_l = bi.cpu().numpy(), bl.cpu().numpy()
    lens = set()
    for j, (r, start, length, e, cursor, _) in enumerate(jobs[:-4]):
        want = start + _perm(r, e, length)[cursor:cursor + b_max]
        assert got_l[j] == len(want) == min(b_max, length - cursor), (j, jobs[j])
        assert np.array_equal(got_i[j, :len(want)], want), (j, jobs[j])
        assert (got_i[j, len(want):] == FILL).all(), (j, jobs[j])    # the sentinel stays
        lens.add(len(want))
    assert b_max in lens and (b_max == 1 or len(lens) > 1)             # full and short batches occurred
    assert (got_l[-4:] == 0).all() and (got_i[-4:] == FILL).all()
    # every length <= 8192: bit for bit niidmix::draw_batches on the same jobs
    k = 3 * len(SHORT)
    di, dl = torch.full_like(bi[:k], FILL), torch.full_like(bl[:k], FILL)
    torch.ops.niidmix.draw_batches(SEED, col(0)[:k], col(1)[:k], col(2)[:k], col(3)[:k], col(4)[:k], di, dl)
    assert torch.equal(di, bi[:k]) and torch.equal(dl, bl[:k])


def test_ops_refuse_wrong_tensors(gpu):
    from niidmix import ops
    v = lambda dt=torch.int32, n=3: torch.zeros(n, dtype=dt, device=gpu)          # noqa: E731
    need = ops.epoch_perm_scratch_bytes(3, 9000)
    assert need == 3 * 16384 * 8
    ok = [v(), v(), v(), v(torch.int64), 9000, v(n=30000), torch.empty(need, dtype=torch.uint8, device=gpu)]
    torch.ops.niidmix.epoch_perm(SEED, *ok)                # zero lengths: nothing is written
    wide = torch.zeros(3, 2, dtype=torch.int32, device=gpu)
    for pos, bad in ((1, v(torch.int64)), (2, v().cpu()), (3, v(n=4)), (3, wide[:, 0]), (4, v()),
                     (5, 0), (5, ops.epoch_perm_max_len() + 1), (6, v(n=30000).float()), (6, v(n=0)),
                     (6, ok[0]), (6, torch.zeros(2, 4, dtype=torch.int32, device=gpu)),
                     (7, torch.empty(need - 1, dtype=torch.uint8, device=gpu)), (7, ok[5]),
                     (7, torch.empty(need, dtype=torch.uint8).pin_memory())):
        args = list(ok)
        args[pos - 1] = bad
        with pytest.raises(RuntimeError):
            torch.ops.niidmix.epoch_perm(SEED, *args)
    bi = torch.zeros(3, 4, dtype=torch.int32, device=gpu)
    ok = [v(n=100), v(torch.int64), v(), v(), v(), bi, v()]
    torch.ops.niidmix.take_batches(*ok)
    for pos, bad in ((1, v(n=100).long()), (1, v(n=0)), (2, v()), (3, v().cpu()), (4, v(n=4)), (5, wide[:, 1]),
                     (6, bi.t().contiguous().t()), (6, bi.float()), (6, bi[0]), (7, ok[2]), (7, v()[:2]),
                     (1, bi.view(-1))):
        args = list(ok)
        args[pos - 1] = bad
        with pytest.raises(RuntimeError):
            torch.ops.niidmix.take_batches(*args)


# ------------------------------------------------------------------------------------------------
# whole rounds
class Linear6(torch.nn.Module):
    K, C = 6, 3

    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(self.K, self.C)

    def forward(self, x, params):
        return torch.nn.functional.log_softmax(self.fc(x.view(-1, self.K)), dim=1)


#         model, sample shape, classes, samples per node, batch, rounds, lr, flags, topology
CASES = {
    "linear": (Linear6, (6,), 3, (9000, 9000, 50), 4000, 7, 0.1, ("device-training",), "ring"),
    "sample": (Linear6, (6,), 3, (9000, 9000, 50), 4000, 7, 0.1,
               ("device-training", "device-training-sample"), "sample"),
    "gn-lenet": (tgs.GN, (1, 15, 15), 3, (4, 8200, 4, 4), 2, 2, 0.05,
                 ("device-training", "device-training-gn-lenet"), "ring"),
}
_data = {}


def _dataset(case):
    if case not in _data:
        _, shape, c, sizes = CASES[case][:4]
        g = torch.Generator().manual_seed(78)
        x = torch.randn(sum(sizes), *shape, generator=g)
        _data[case] = (x, torch.randint(0, c, (sum(sizes),), generator=g))
    return _data[case]


def _run(case, cached, momentum, monkeypatch, budget=None):
    """The plugin's rounds under --device-sampling-cached (`cached`) or on the existing round fed
    the restatement's batches.  Returns the per-round log."""
    from niidmix import d_sgd, train
    from niidmix.sampling import SamplerState
    model, _, _, sizes, batch, rounds, lr, flags, topology = CASES[case]
    n = len(sizes)
    monkeypatch.setattr(d_sgd, "_sample_cache", {})
    if not cached:
        monkeypatch.setattr(train, "index_loader", tgsamp._restated_loader)
    if budget is not None:
        monkeypatch.setattr(train.DeviceTrainer, "_budget", lambda self: budget)
    params = {"meta": {"log": "WARNING", "seed": SEED}, "nodes": {"nb-nodes": n},
              "topology": {"name": "sample", "sample-method": "random-with-overlap", "sample-size": 2,
                           "sample-overlap": 1} if topology == "sample" else
              {"name": "ring", "remove-clique-edges": 0},
              "logger": {"accuracy-logging-interval": 0, "accuracy-logging-interval-steps": 0,
                         "log-consensus-distance": False},
              "algorithm": {"learning-rate": lr, "learning-momentum": momentum, "batch-size": batch,
                            "initial-averaging": False, "clique-gradient": False,
                            "unbiased-gradient": False, "deferred-writeback": False,
                            "mixing-mode": "exact", **{f: True for f in flags},
                            **({"device-sampling": True, "device-sampling-cached": True} if cached else {})}}
    x, y = _dataset(case)
    start = np.cumsum([0] + list(sizes))
    torch.manual_seed(2028)
    gen = torch.Generator().manual_seed(2029)
    nodes = []
    for r in range(n):
        mdl = model()
        if case == "gn-lenet":
            tgs.th.perturb(mdl, gen)
        nodes.append({"rank": r, "epoch": 0, "model": mdl, "optimizer": d_sgd.optimizer(mdl, params),
                      "train-set": [(x[j], int(y[j])) for j in range(start[r], start[r + 1])]})
    topo = {"edges": {}, "weights": []} if topology == "sample" else tgsamp._Ring(n).topo
    state, _, _ = d_sgd.init(nodes, topo, params)
    assert all((nd["train-iterator"] is None) == cached for nd in nodes)
    st = SamplerState(range(n), sizes, batch)
    log, calls = [], []
    for k in range(rounds):
        state, losses, done, active = d_sgd.next_step(state, params, None)
        d_sgd.synchronize()
        rows = [nd["rank"] for nd in active]
        epoch, cursor, want_done = st.advance(rows)
        assert done == want_done and [nd["epoch"] for nd in nodes] == st.epoch.tolist(), f"round {k}"
        assert sorted(losses) == sorted(rows) and all(np.isfinite(v) for v in losses.values())
        tr = d_sgd._trainers[id(nodes)]
        assert tr.sampling == tr.cached == cached
        # the index block the gradient op read: the restatement's batches, node offsets added
        bi = tr.layout.view(tr.idx_dev, "indices").cpu().numpy()
        bl = tr.layout.view(tr.idx_dev, "lengths").cpu().numpy()
        for j, (r, e, c) in enumerate(zip(rows, epoch.tolist(), cursor.tolist())):
            want = start[r] + _perm(r, e, sizes[r])[c:c + batch]
            assert bl[j] == len(want) and np.array_equal(bi[j, :len(want)], want), (k, j)
        if cached:
            # sorted: exactly the rows that began an epoch this round
            began = [r for r, c in zip(rows, cursor.tolist()) if c == 0]
            assert tr.last_perm_jobs == len(began), f"round {k}"
            n_long = sum(sizes[r] > 8192 for r in began)
            per_call = n_long if budget is None else 1
            want_calls = (len(began) > n_long) + (-(-n_long // per_call) if n_long else 0)
            assert tr.last_perm_calls == want_calls, f"round {k}"
            calls.append(len(began))
        log.append((rows, losses, done, tgs._flat(nodes)))
    assert any(any(d.values()) for _, _, d, _ in log)                 # an epoch ended on the way
    if cached:
        assert calls[0] == len(log[0][0])                             # round 0 sorts every row it draws
        assert case != "linear" or calls == [3, 1, 1, 3, 1, 1, 3]     # 9000 / 4000: three rounds an epoch
    return log


@pytest.mark.parametrize("case,momentum,budget", [("linear", 0.9, None), ("linear", 0.0, 16384 * 8),
                                                  ("sample", 0.9, None), ("gn-lenet", 0.9, None)])
def test_rounds_equal_the_existing_round_on_the_same_indices(gpu, monkeypatch, case, momentum, budget):
    log_c = _run(case, True, momentum, monkeypatch, budget)
    log_h = _run(case, False, momentum, monkeypatch)
    assert len(log_c) == len(log_h) == CASES[case][5]
    for k, ((rows_c, loss_c, done_c, th_c), (rows_h, loss_h, done_h, th_h)) in enumerate(zip(log_c, log_h)):
        assert rows_c == rows_h and done_c == done_h, f"round {k}"
        assert loss_c == loss_h, f"round {k}"                         # the same floats
        assert torch.equal(th_c.view(torch.int32), th_h.view(torch.int32)), f"round {k}"
    assert not torch.equal(log_c[0][3], log_c[-1][3])                 # and the models moved
