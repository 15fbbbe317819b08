"""--device-sampling-torch-stream on the GPU: niidmix::torch_randperm against torch.randperm on the
CPU, exact equality; the jobs it skips; the C entry's status codes; and whole rounds through
d_sgd.init / next_step that equal, bit for bit, the run without --device-sampling (real loaders on
the global torch generator): index block, losses, epoch counts, parameters and RNG state."""
import numpy as np
import pytest
import torch

import test_gpu_sampling as tgsamp
import test_gpu_train_sample as tgs

pytestmark = pytest.mark.gpu

# the edges of the twist's stretches (227, 454), of a block of 624 draws at n - 1, of what the
# trainer calls a short row (8192), and the uint16 limit
LENGTHS = (1, 2, 3, 63, 64, 65, 227, 228, 624, 625, 1248, 1249, 8192, 8193, 65536)
SEEDS = (0, 1, 2 ** 31, 2 ** 32 - 1)
FILL = -7
_want = {}


def _randperm(seed, n):
    """torch.randperm on the CPU, computed once per (seed, n)."""
    if (seed, n) not in _want:
        _want[seed, n] = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).numpy()
    return _want[seed, n]


def _as_i32(seeds):
    return np.asarray(seeds, dtype=np.uint32).view(np.int32).tolist()


def _dev(gpu, v, dt=torch.int32):
    return torch.tensor(v, dtype=dt, device=gpu)


def test_kernel_equals_torch_randperm(gpu):
    from niidmix import ops  # noqa: F401  (registers torch.ops.niidmix.*)
    jobs = [(s, n) for n in LENGTHS for s in SEEDS]
    m = len(jobs)
    # the stretches in another order than the jobs, with gaps between, before and after them
    off, at = [0] * m, 5
    for j in sorted(range(m), key=lambda j: (7 * j + 3) % m):
        off[j] = at
        at += jobs[j][1] + 2 + j % 5
    size = at + 11
    args = (_dev(gpu, _as_i32([s for s, _ in jobs])), _dev(gpu, [n for _, n in jobs]),
            _dev(gpu, off, torch.int64), max(LENGTHS))
    perm = torch.full((size,), FILL, dtype=torch.int32, device=gpu)
    torch.ops.niidmix.torch_randperm(*args, perm)
    got = perm.cpu().numpy()
    untouched = np.ones(size, dtype=bool)
    for j, (s, n) in enumerate(jobs):
        assert np.array_equal(got[off[j]:off[j] + n], _randperm(s, n)), (s, n)
        untouched[off[j]:off[j] + n] = False
    assert untouched.sum() >= 2 * m and (got[untouched] == FILL).all()        # the sentinel stays
    again = torch.full_like(perm, FILL)
    torch.ops.niidmix.torch_randperm(*args, again)
    assert torch.equal(again, perm)                                           # two calls, the same bits
    # the seed's high bits do not count: the CPU's permutation for 2^32 + 7 is the one for 7
    one = torch.full((1300,), FILL, dtype=torch.int32, device=gpu)
    torch.ops.niidmix.torch_randperm(_dev(gpu, [7]), _dev(gpu, [1249]), _dev(gpu, [20], torch.int64), 1249, one)
    assert np.array_equal(one.cpu().numpy()[20:1269], _randperm(2 ** 32 + 7, 1249))


def test_kernel_skips_what_it_cannot_write(gpu):
    """seg_len 0 or negative, seg_len above max_len, a stretch that runs past perm or starts before
    it: each leaves the sentinel; the jobs beside them are written."""
    from niidmix import ops  # noqa: F401  (registers torch.ops.niidmix.*)
    lengths = (0, 300, 70, -4, 50, 50, 64)
    off = (0, 400, 10, 100, 960, -1, 900)              # job 4 runs past the end, job 5 starts before it
    size, max_len = 1000, 299                          # job 1 is longer than max_len
    perm = torch.full((size,), FILL, dtype=torch.int32, device=gpu)
    torch.ops.niidmix.torch_randperm(_dev(gpu, [3] * 7), _dev(gpu, lengths), _dev(gpu, off, torch.int64),
                                     max_len, perm)
    got = perm.cpu().numpy()
    untouched = np.ones(size, dtype=bool)
    for j in (2, 6):
        assert np.array_equal(got[off[j]:off[j] + lengths[j]], _randperm(3, lengths[j])), j
        untouched[off[j]:off[j] + lengths[j]] = False
    assert (got[untouched] == FILL).all()
    # a stretch that ends exactly at perm_len is inside
    torch.ops.niidmix.torch_randperm(_dev(gpu, [3]), _dev(gpu, [50]), _dev(gpu, [950], torch.int64), 50, perm)
    assert np.array_equal(perm.cpu().numpy()[950:], _randperm(3, 50))


def test_argument_checks_come_before_any_launch(gpu):
    """The documented codes in the documented order, on made-up addresses that are never
    dereferenced; and the op's own refusals."""
    from niidmix import _lib, ops
    L = _lib.lib
    F = L.niidmix_torch_randperm_i32
    most = L.niidmix_torch_randperm_max_len()
    assert most == ops.torch_randperm_max_len() == 65536
    n, length, plen = 3, 2000, 70000
    A = [(i + 1) << 24 for i in range(4)]                 # seed_lo, seg_len, perm_off, perm
    names = ("seed_lo", "seg_len", "perm_off", "perm")

    def call(n_jobs=n, max_len=length, perm_len=plen, **ptr):
        a = [ptr.get(k, v) for k, v in zip(names, A)]
        return F(a[0], a[1], a[2], n_jobs, max_len, a[3], perm_len, None)

    for name in names:
        assert call(**{name: None}) == _lib.EINVAL and b"null" in L.niidmix_last_error(), name
    assert call(seed_lo=None, n_jobs=0) == _lib.EINVAL and b"null" in L.niidmix_last_error()
    assert call(n_jobs=0) == _lib.EINVAL and call(n_jobs=-1) == _lib.EINVAL
    assert call(max_len=0) == _lib.EINVAL and call(max_len=-5) == _lib.EINVAL and call(perm_len=0) == _lib.EINVAL
    assert call(n_jobs=0, max_len=most + 1) == _lib.EINVAL                 # sizes before limits
    assert call(max_len=most + 1) == _lib.EUNSUPPORTED and b"max_len" in L.niidmix_last_error()
    assert call(n_jobs=1 << 31) == _lib.EUNSUPPORTED
    assert call(max_len=most + 1, seed_lo=A[3]) == _lib.EUNSUPPORTED       # limits before aliasing
    for name, words in (("seed_lo", n), ("seg_len", n), ("perm_off", 2 * n)):
        assert call(**{name: A[3] + 4 * (plen - 1)}) == _lib.EALIAS, name        # an input inside perm
        assert call(**{name: A[3] - 4 * (words - 1)}) == _lib.EALIAS, name       # its tail on perm's head
    # (no call above passes every check: that one would launch on the made-up addresses)
    # the op
    v = lambda dt=torch.int32, k=3: torch.zeros(k, dtype=dt, device=gpu)           # noqa: E731
    ok = [v(), v(), v(torch.int64), 100, v(k=500)]
    torch.ops.niidmix.torch_randperm(*ok)                  # zero lengths: nothing is written
    assert not ok[4].any()
    wide = torch.zeros(3, 2, dtype=torch.int32, device=gpu)
    for pos, bad in ((0, v(torch.int64)), (0, v().cpu()), (1, v(k=4)), (1, wide[:, 0]), (2, v()), (3, 0),
                     (3, most + 1), (4, v(k=500).float()), (4, v(k=0)), (4, ok[0]), (4, v(k=500).cpu())):
        args = list(ok)
        args[pos] = bad
        with pytest.raises(RuntimeError):
            torch.ops.niidmix.torch_randperm(*args)


# ------------------------------------------------------------------------------------------------
# whole rounds
class Linear8(torch.nn.Module):
    K, C = 8, 3

    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(self.K, self.C)

    def forward(self, x, params):
        return torch.nn.functional.log_softmax(self.fc(x.view(-1, self.K)), dim=1)


SIZES, BATCH, ROUNDS = (5, 7, 4, 10, 3), 3, 9
_data = []


def _dataset():
    if not _data:
        g = torch.Generator().manual_seed(83)
        x = torch.randn(sum(SIZES), Linear8.K, generator=g)
        _data.append((x, torch.randint(0, Linear8.C, (sum(SIZES),), generator=g)))
    return _data[0]


def _run(sample, momentum, flagged, monkeypatch):
    """ROUNDS rounds of the plugin under --device-training (and --device-training-sample), on the
    device's torch stream (`flagged`) or on real index loaders.  Returns the per-round log, the
    nodes' epochs, the final parameters and the global generator's state."""
    from niidmix import d_sgd
    from niidmix.sampling import SamplerState
    n = len(SIZES)
    monkeypatch.setattr(d_sgd, "_sample_cache", {})
    flags = ("device-training",) + (("device-training-sample",) if sample else ()) + \
        (("device-sampling", "device-sampling-torch-stream") if flagged else ())
    params = {"meta": {"log": "WARNING"}, "nodes": {"nb-nodes": n},
              "topology": {"name": "sample", "sample-method": "random", "sample-size": 2} if sample else
              {"name": "ring", "remove-clique-edges": 0},
              "logger": {"accuracy-logging-interval": 0, "accuracy-logging-interval-steps": 0,
                         "log-consensus-distance": False},
              "algorithm": {"learning-rate": 0.1, "learning-momentum": momentum, "batch-size": BATCH,
                            "initial-averaging": False, "clique-gradient": False,
                            "unbiased-gradient": False, "deferred-writeback": False,
                            "mixing-mode": "exact", **{f: True for f in flags}}}
    x, y = _dataset()
    start = np.cumsum([0] + list(SIZES))
    torch.manual_seed(2030)
    nodes = []
    for r in range(n):
        mdl = Linear8()
        nodes.append({"rank": r, "epoch": 0, "model": mdl, "optimizer": d_sgd.optimizer(mdl, params),
                      "train-set": [(x[j], int(y[j])) for j in range(start[r], start[r + 1])]})
    topo = {"edges": {}, "weights": []} if sample else tgsamp._Ring(n).topo
    state, _, _ = d_sgd.init(nodes, topo, params)
    assert all((nd["train-iterator"] is None) == flagged for nd in nodes)
    st = SamplerState(range(n), SIZES, BATCH)
    log = []
    for k in range(ROUNDS):
        state, losses, done, active = d_sgd.next_step(state, params, None)
        d_sgd.synchronize()
        rows = [nd["rank"] for nd in active]
        tr = d_sgd._trainers[id(nodes)]
        assert tr.sampling == tr.cached == tr.torch_stream == flagged
        _, cursor, want_done = st.advance(rows)
        assert done == want_done and [nd["epoch"] for nd in nodes] == st.epoch.tolist(), f"round {k}"
        bi = tr.layout.view(tr.idx_dev, "indices").cpu().numpy()
        bl = tr.layout.view(tr.idx_dev, "lengths").cpu().numpy()[:len(rows)].tolist()
        assert bl == [min(BATCH, SIZES[r] - c) for r, c in zip(rows, cursor.tolist())], f"round {k}"
        if flagged:
            # shuffled: exactly the rows that began an epoch this round, in one call (all are short)
            began = sum(c == 0 for c in cursor.tolist())
            assert tr.last_perm_jobs == began and tr.last_perm_calls == (began > 0), f"round {k}"
        log.append((rows, [bi[j, :b].tolist() for j, b in enumerate(bl)], bl, losses, done))
    assert any(any(d.values()) for *_, d in log)                          # epochs ended on the way
    return log, [nd["epoch"] for nd in nodes], tgs._flat(nodes), torch.get_rng_state()


@pytest.mark.parametrize("sample,momentum", [(False, 0.0), (True, 0.0), (False, 0.9)],
                         ids=["graph", "sample", "graph-momentum"])
def test_rounds_equal_the_run_on_real_loaders(gpu, monkeypatch, sample, momentum):
    log_d, epochs_d, theta_d, rng_d = _run(sample, momentum, True, monkeypatch)
    log_h, epochs_h, theta_h, rng_h = _run(sample, momentum, False, monkeypatch)
    assert len(log_d) == len(log_h) == ROUNDS
    for k, (d, h) in enumerate(zip(log_d, log_h)):
        assert d[0] == h[0], f"round {k}: active rows"
        assert d[1] == h[1] and d[2] == h[2], f"round {k}: indices and lengths of the index block"
        assert d[3] == h[3], f"round {k}: losses"                          # the same floats
        assert d[4] == h[4], f"round {k}: epoch_done"
    assert epochs_d == epochs_h and max(epochs_d) >= 1
    assert torch.equal(theta_d.view(torch.int32), theta_h.view(torch.int32))
    assert torch.equal(rng_d, rng_h)
    assert all(len(d[0]) == (2 if sample else len(SIZES)) for d in log_d)
