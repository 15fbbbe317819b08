"""The GN-LeNet kernels where include/niidmix.h's promises end and where no other test goes: the
largest shapes (64 x 64, Cin 4, C 1024), the matrix-core kernel's own limit and its elongated
shapes, gradient batches of five tiles and of none, and the second trip of the persistent loops of
k_gnl_eval (both variants) and k_gnl_eval_mfma.

Yardsticks are those of tests/test_gpu_eval_gnlenet.py and tests/test_gpu_train_gnlenet.py, which
reason them: logits within 4 e32 of float64, the loss within 2 * 4 e32 * len, pred the float64
argmax outside a 16 e32 gap (at most 1 % of a case's pairs inside it); per-tensor gradients and the
loss within 4 e32, every gradient case separated (pool gaps and pre-ReLU magnitudes > 16 e_act).
tests/test_gnlenet_limits_host.py checks every seeded case's ambiguity and separation, the tile rule
this file relies on and the M-tile coverage without a GPU.

k_gnl_grad_sample's persistent loop (the same 2^20 cap) is not exercised: a scratch slot per work
item makes 2^20 + 1 items cost tens of GB.
"""
import functools
import math

import pytest
import torch

import test_eval_gnlenet_host as th
import test_gpu_eval_gnlenet as tg
from test_gpu_train_gnlenet import (_check_accuracy, _check_sentinels, _launch as launch_grad,
                                    add_references, make_case, separation)

pytestmark = pytest.mark.gpu

M, N_ROWS = 12, 3
PLAIN, MFMA = "gnlenet_eval_rows", "gnlenet_eval_rows_mfma"

# Samples per tile of k_gnl_eval_mfma (ops.gn_mfma_tile; the host file checks these against the
# library) and, from them, the M-tiles of 32 output positions a wave owns in conv2 (pooled map
# h1 x w1) and conv3 (h2 x w2): n_mt = ceil(tile h w / 32), wave v of 4 owns (n_mt - v + 3) // 4 of
# them, none when v >= n_mt.  A count selects gn_mma_pick's instantiation.
#
#   H x W    tile   h1 x w1  n_mt  conv2 counts   h2 x w2  n_mt  conv3 counts   tested in
#   15 x 15    4     7 x 7     7   2 2 2 1         3 x 3     2   1 1 0 0        both files
#   17 x 15    4     8 x 7     7   2 2 2 1         3 x 3     2   1 1 0 0        test_gpu_eval_gnlenet_mfma
#   28 x 28    4    13 x 13   22   6 6 5 5         6 x 6     5   2 1 1 1        both files
#   32 x 32    2    15 x 15   15   4 4 4 3         7 x 7     4   1 1 1 1        test_gpu_eval_gnlenet_mfma
#   42 x 42    2    20 x 20   25   7 6 6 6         9 x 9     6   2 2 1 1        this file
#   44 x 15    4    21 x 7    19   5 5 5 4        10 x 3     4   1 1 1 1        this file
#   64 x 15    2    31 x 7    14   4 4 3 3        15 x 3     3   1 1 1 0        this file
#
# conv2: 1 .. 7 (7 only at 42 x 42), conv3: 0, 1, 2: no hole, so no further shape.
MFMA_TILE = {(15, 15): 4, (17, 15): 4, (28, 28): 4, (32, 32): 2, (42, 42): 2, (44, 15): 4, (64, 15): 2}
MFMA_SHAPES = [(2, 42, 42, 10), (1, 44, 15, 10), (1, 64, 15, 10), (4, 28, 28, 10), (1, 15, 15, 1024),
               (1, 15, 15, 257)]
MFMA_REFUSED = (2, 42, 43, 10)
# the scratch-slot variant at the limit of H, W and Cin; ev_scan and gn_linear at the limit of C and
# at a C that is 1 past a multiple of the 4 waves and of the wave size
PLAIN_SHAPES = [(4, 64, 64, 10), (1, 15, 15, 1024), (1, 15, 15, 257)]
EVAL = [(PLAIN, s) for s in PLAIN_SHAPES] + [(MFMA, s) for s in MFMA_SHAPES]
LOOP_SHAPE = (1, 15, 15, 3)
# K = 7 job patterns (slab row, start, length <= tile) per tile size: 2^k mod 7 is never 0, so a
# workgroup's second item (job + a power-of-two grid) is another pattern than its first
PATTERNS = {2: [(0, 0, 2), (1, 0, 1), (2, 1, 2), (0, 3, 1), (1, 4, 2), (2, 6, 1), (1, 2, 2)],
            4: [(0, 0, 4), (1, 0, 1), (2, 1, 3), (0, 3, 2), (1, 4, 4), (2, 6, 1), (1, 2, 3)]}
SLOT_CAP, GRID_CAP = 4096, 1 << 20         # kGnMaxSlots, kGnMaxGrid


def _down(h):
    return (h - 3) // 2 + 1


def wave_tile_counts(hw, tile):
    """({conv2 counts}, {conv3 counts}) over the 4 waves at H x W inputs: the rule above."""
    def counts(m):
        n_mt = -(-m // 32)
        return {(n_mt - v + 3) // 4 if v < n_mt else 0 for v in range(4)}
    h1, w1 = _down(hw[0]), _down(hw[1])
    return counts(tile * h1 * w1), counts(tile * _down(h1) * _down(w1))


def check_mtile_coverage():
    conv2, conv3 = set(), set()
    for hw, tile in MFMA_TILE.items():
        a, b = wave_tile_counts(hw, tile)
        conv2 |= a
        conv3 |= b
    assert {s[1:3] for s in MFMA_SHAPES + [LOOP_SHAPE]} <= set(MFMA_TILE)
    assert conv2 == set(range(1, 8)), f"conv2's per-wave M-tile counts under test: {sorted(conv2)}"
    assert conv3 == {0, 1, 2}, f"conv3's per-wave M-tile counts under test: {sorted(conv3)}"
    assert 7 in wave_tile_counts((42, 42), 2)[0]


def tile_of(op, shape):
    return MFMA_TILE[shape[1:3]] if op == MFMA else tg.TS


def jobs_of(t):
    """(slab row, start, length): lengths 2 T + 1, T + 1, T, 1 and 0; jobs 0 and 1 share a start,
    rows 0 and 1 are listed twice."""
    return [(0, 0, 2 * t + 1), (1, 0, t + 1), (2, 3, t), (0, 5, 1), (1, 2, 0)]


def slot_shape():
    """The smallest square input at which k_gnl_eval's activations leave LDS for scratch slots,
    found through the size function (one work item needs 16 bytes of partial sums besides)."""
    from niidmix._lib import lib
    for h in range(15, 65):
        if lib.niidmix_gnlenet_eval_rows_scratch_bytes(1, 1, 1, h, h, 3) > 16:
            return (1, h, h, 3)
    raise AssertionError("no shape has activation slots")


@functools.lru_cache(None)
def eval_case(op, shape, seed):
    """Inputs and the float64 / fp32 CPU logits of N_ROWS models on M samples, once."""
    cin, h, w, c = shape
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    theta = torch.stack([torch.cat([q.detach().reshape(-1) for q in
                                    th.perturb(th.GNLeNet(cin, c, (h, w)), gen).parameters()])
                         for _ in range(N_ROWS)])
    x = torch.randn(M, cin, h, w, generator=gen)
    y = torch.randint(0, c, (M,), generator=gen)
    z64 = torch.stack([th.forward_logits(theta[r], x, c, torch.float64) for r in range(N_ROWS)])
    z32 = torch.stack([th.forward_logits(theta[r], x, c, torch.float32) for r in range(N_ROWS)])
    return dict(op=op, shape=shape, theta=theta, x=x, y=y, z64=z64, z32=z32, p=theta.shape[1])


def limit_case(i):
    op, shape = EVAL[i]
    return eval_case(op, shape, 3000 + i), jobs_of(tile_of(op, shape))


def loop_case(op, shape):
    return eval_case(op, shape, 3100 + (op == MFMA) + 2 * (shape != LOOP_SHAPE)), PATTERNS[tile_of(op, shape)]


def yardstick(d, jobs):
    """(e32, ambiguous pairs, pairs) of a case's jobs: torch's fp32 CPU error on the samples the
    jobs score, and how many (job, sample) pairs have a float64 top-two gap within 16 e32."""
    e32 = max(float((d["z32"][r, s:s + n].double() - d["z64"][r, s:s + n]).abs().max()) for r, s, n in jobs if n)
    ambiguous = pairs = 0
    for r, s, n in jobs:
        if n and d["shape"][3] > 1:
            top = d["z64"][r, s:s + n].topk(2, dim=1).values
            ambiguous += int(((top[:, 0] - top[:, 1]) <= 16 * e32).sum())
        pairs += n
    return e32, ambiguous, pairs


def launch_eval(d, dev, jobs, layout="vec", logits=True, timed=False):
    """The case's op on `jobs`, a list of (row, start, length) or three int32 device tensors.
    Returns (loss_sum, correct, pred, logits, slab before, after) on the CPU, sentinels -7 in pred
    and logits with two spare columns; logits=False passes none (None is returned); `timed`: the
    launch's milliseconds appended."""
    from niidmix import ops  # noqa: F401  (registers the ops)
    cin, h, w, c = d["shape"]
    p = d["p"]
    ld = (p + 3) // 4 * 4 if layout == "vec" else p + 1
    slab = torch.zeros(N_ROWS + 1, ld, device=dev)
    slab[:N_ROWS, :p] = d["theta"].to(dev)
    before = slab.clone()
    if not torch.is_tensor(jobs[0]):
        jobs = [torch.tensor([j[i] for j in jobs], dtype=torch.int32, device=dev) for i in range(3)]
    n, max_len = jobs[0].numel(), max(int(jobs[2].max()), 1)
    loss = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
    correct = torch.full((n,), -1, dtype=torch.int32, device=dev)
    pred = torch.full((n, max_len + 2), -7, dtype=torch.int32, device=dev)
    z = torch.full((n, max_len + 2, c), -7.0, dtype=torch.float32, device=dev) if logits else None
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    getattr(torch.ops.niidmix, d["op"])(
        slab[:, :p], d["x"].reshape(M, -1).to(dev), d["y"].to(torch.int32).to(dev), *jobs, max_len, loss,
        correct, pred[:, :max_len], z, cin, h, w, c)
    t1.record()
    torch.cuda.synchronize()
    out = (loss.cpu(), correct.cpu(), pred.cpu(), z.cpu() if logits else None, before.cpu(), slab.cpu())
    return out + (t0.elapsed_time(t1),) if timed else out


def check_eval(d, jobs, out, what):
    """A launch with logits against float64 under tests/test_gpu_eval_gnlenet.py's bounds."""
    loss, correct, pred, logits, before, after = out
    c = d["shape"][3]
    e32, ambiguous, pairs = yardstick(d, jobs)
    assert ambiguous <= 0.01 * pairs, "the case is ambiguous in float64: reseed it"
    assert torch.equal(tg._bits(before), tg._bits(after)), "theta was written"
    worst = 0.0
    for i, (r, s, n) in enumerate(jobs):
        assert bool((pred[i, n:] == -7).all()) and bool((logits[i, n:] == -7.0).all()), "past seg_len"
        if n == 0:
            assert float(loss[i]) == 0.0 and int(correct[i]) == 0
            continue
        z64, y = d["z64"][r, s:s + n], d["y"][s:s + n]
        worst = max(worst, float((logits[i, :n].double() - z64).abs().max()))
        pr = pred[i, :n].long()
        assert bool(((pr >= 0) & (pr < c)).all())
        top = z64.topk(2, dim=1).values if c > 1 else torch.tensor([[1.0, 0.0]]).expand(n, 2)
        amb = (top[:, 0] - top[:, 1]) <= 16 * e32
        assert bool((pr[~amb] == z64.argmax(1)[~amb]).all()), "pred differs from the float64 argmax"
        for k in amb.nonzero().flatten().tolist():
            assert float(z64[k].max() - z64[k, pr[k]]) <= 16 * e32
        assert int(correct[i]) == int((pr == y).sum())
        nll = torch.logsumexp(z64, 1) - z64[torch.arange(n), y]
        assert abs(float(loss[i]) - float(nll.sum())) <= 2 * 4 * e32 * n
    print(f"{what}: e32 {e32:.3g}  kernel max |z - z64| {worst:.3g}  ratio {worst / e32:.3g}")
    assert worst <= 4 * e32, f"kernel logits off by {worst:.3g} = {worst / e32:.3g} e32"


_eval_ids = [f"{'mfma' if op == MFMA else 'plain'}-{'x'.join(map(str, s))}" for op, s in EVAL]


@pytest.mark.parametrize("layout", ["vec", "odd"])
@pytest.mark.parametrize("i", range(len(EVAL)), ids=_eval_ids)
def test_evaluation_at_the_limits(i, layout, gpu):
    d, jobs = limit_case(i)
    check_eval(d, jobs, launch_eval(d, gpu, jobs, layout=layout), f"{_eval_ids[i]} {layout}")


def test_mtile_counts_under_test_cover_every_instantiation():
    check_mtile_coverage()


def test_tile_position_at_the_tile_2_limit(gpu):
    """(2, 42, 42, 10), 7 M-tiles in wave 0: a sample scored alone has the logit bits it has at any
    position of the job of 2 T + 1."""
    i = EVAL.index((MFMA, (2, 42, 42, 10)))
    d, jobs = limit_case(i)
    n = jobs[0][2]
    a = launch_eval(d, gpu, jobs)
    single = launch_eval(d, gpu, [(0, s, 1) for s in range(n)])
    for s in range(n):
        assert torch.equal(tg._bits(single[3][s, 0]), tg._bits(a[3][0, s])), s
        assert int(single[2][s, 0]) == int(a[2][0, s])


def test_one_column_past_the_mfma_limit_is_unsupported(gpu):
    from niidmix import _lib, ops
    cin, h, w, c = MFMA_REFUSED
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=gpu)  # noqa: E731
    with pytest.raises(_lib.NiidmixError, match=f"niidmix error {_lib.EUNSUPPORTED}.*matrix-core"):
        torch.ops.niidmix.gnlenet_eval_rows_mfma(
            torch.zeros(1, ops.gnlenet_sizes(*MFMA_REFUSED)[1], device=gpu),
            torch.zeros(2, cin * h * w, device=gpu), i32(0).repeat(2), i32(0), i32(0), i32(2), 2,
            torch.empty(1, dtype=torch.float64, device=gpu), i32(0), None, None, cin, h, w, c)


# ------------------------------------------------------------------------------------------------
# the second trip of the persistent loops
def _second_trips(op, shape, n_jobs, cap, gpu):
    """n_jobs > cap one-tile jobs cycling through the 7 patterns: every job has the loss bits, the
    count and the predictions that its pattern has in a launch of the 7 alone, which is checked
    against float64.  Prints the long launch's milliseconds."""
    d, pats = loop_case(op, shape)
    assert n_jobs > cap and cap & (cap - 1) == 0 and len(pats) == 7
    small = launch_eval(d, gpu, pats)
    check_eval(d, pats, small, f"{op} {shape} 7 patterns")
    sel = torch.arange(n_jobs, device=gpu) % 7
    cols = torch.tensor(pats, dtype=torch.int32, device=gpu)[sel]
    big = launch_eval(d, gpu, [cols[:, i].contiguous() for i in range(3)], logits=False, timed=True)
    sel = sel.cpu()
    assert torch.equal(tg._bits(big[4]), tg._bits(big[5])), "theta was written"
    bad = (tg._bits(big[0]) != tg._bits(small[0])[sel]) | (big[1] != small[1][sel]) | \
        (big[2] != small[2][sel]).any(1)
    first = int(bad.nonzero()[0]) if bool(bad.any()) else -1
    assert first < 0, f"{int(bad.sum())} of {n_jobs} jobs differ from their pattern, the first is job {first}"
    print(f"{op} {shape}: {n_jobs} jobs in {big[6]:.1f} ms")


def test_second_trip_of_the_scratch_slot_loop(gpu):
    _second_trips(PLAIN, slot_shape(), SLOT_CAP + 300, SLOT_CAP, gpu)


@pytest.mark.parametrize("op", [PLAIN, MFMA])
def test_second_trip_of_the_lds_loops(op, gpu):
    _second_trips(op, LOOP_SHAPE, GRID_CAP + 300, GRID_CAP, gpu)


# ------------------------------------------------------------------------------------------------
# the gradient.  The samples of the 64 x 64 case were taken one at a time from a seeded pool
# (pool_sample; row r looks at numbers r BIG_POOL and up), a sample being kept when its row's batch
# stays separated with it (pick_separated): of some 40 000 pool windows and as many ReLU inputs a
# sample, about one random sample in 500 is separated.  The other seeds are the first from their
# base (a multiple of 100) that separate.
BIG = (4, 64, 64, 10, 2, 2, (2, 1), 4100)
BIG_POOL = 4096
BIG_PICK = ((1575, 2042), (4884,))        # per row: the pool numbers of its batch
GRAD = {"wide": (1, 15, 15, 1024, 1, 2, (2,), 4200),
        "long": (1, 15, 15, 3, 3, 9, (9, 6, 1), 4313),
        "zero": (1, 15, 15, 3, 3, 3, (3, 0, 2), 4401)}


def pool_sample(k):
    """Sample k of the 64 x 64 case's pool."""
    return torch.randn(BIG[:3], generator=torch.Generator().manual_seed(BIG[7] + 1 + k))


def pick_separated(theta_row, r, n):
    """The first n pool numbers of row r, in order, whose batch stays separated as it grows."""
    got, xs = [], []
    for k in range(r * BIG_POOL, (r + 1) * BIG_POOL):
        e_act, gap, mag = separation(theta_row, torch.stack(xs + [pool_sample(k)]))
        if gap > 16 * e_act and mag > 16 * e_act:
            got.append(k)
            xs.append(pool_sample(k))
            if len(got) == n:
                return got
    raise AssertionError("the pool is exhausted: reseed the case")


def _live(d, rows):
    """The case restricted to `rows` (entries with samples), for the references: same samples."""
    return dict(d, n_rows=len(rows), theta=d["theta"][rows], idx=d["idx"][rows],
                lens=[d["lens"][r] for r in rows])


@functools.lru_cache(None)
def grad_case(name):
    """A case with its float64 / fp32 references; "zero": those of rows 0 and 2 under "live"."""
    if name == "big":
        take = [k for row in BIG_PICK for k in row]
        take.append(next(k for k in range(4) if k not in take))       # fills row 1's idx, not read
        x = torch.stack([pool_sample(k) for k in take])
        return add_references(dict(make_case(*BIG), x=x, idx=torch.tensor([[0, 1], [2, 3]])))
    d = make_case(*GRAD[name])
    if name == "zero":
        return dict(d, live=add_references(_live(d, [0, 2])))
    return add_references(d)


def assert_separated(d):
    for r in range(d["n_rows"]):
        if d["lens"][r] == 0:
            continue
        ix = d["idx"][r, :d["lens"][r]]
        e_act, gap, mag = separation(d["theta"][r], d["x"][ix])
        assert gap > 16 * e_act and mag > 16 * e_act, \
            f"reseed the case: e_act {e_act:.3g}, pool gap {gap:.3g}, pre-ReLU magnitude {mag:.3g}"


def _row_bits_equal(d, a, b, r, k):
    """Row r of launch a against entry k of launch b: gradient and loss bits."""
    p, perm = d["p"], a[2]
    return torch.equal(tg._bits(a[0][perm[r], :p]), tg._bits(b[0][perm[r], :p])) and \
        torch.equal(tg._bits(a[1][r]), tg._bits(b[1][k]))


@pytest.mark.parametrize("layout", ["vec", "odd"])
@pytest.mark.parametrize("name", ["big", "wide", "long"])
def test_gradient_at_the_limits(name, layout, gpu):
    """64 x 64 with Cin 4 (k_gnl_grad_conv's 31 x 31 maps); C 1024; five tiles, the last half full."""
    from niidmix import ops  # noqa: F401  (registers the op)
    d = grad_case(name)
    assert_separated(d)
    grad, loss, perm, before, after = launch_grad(d, gpu, layout=layout)
    _check_sentinels(d, grad, perm, before, after)
    _check_accuracy(d, grad, loss, perm, f"{name} {'x'.join(map(str, d['shape']))} {layout}")


def test_long_batch_rows_alone(gpu):
    """Lengths (9, 6, 1): each row launched alone has the bits it has among the others."""
    from niidmix import ops  # noqa: F401
    d = grad_case("long")
    a = launch_grad(d, gpu)
    for r in range(d["n_rows"]):
        assert _row_bits_equal(d, a, launch_grad(d, gpu, order=[r]), r, 0), r


@pytest.mark.parametrize("layout", ["vec", "odd"])
def test_a_row_of_length_zero(layout, gpu):
    """Lengths (3, 0, 2): row 1 gets a NaN loss and an exactly zero gradient in all P columns; rows
    0 and 2 are within 4 e32 of float64 and have the bits of a launch without row 1."""
    from niidmix import ops  # noqa: F401
    d = grad_case("zero")
    assert_separated(d)
    p = d["p"]
    a = launch_grad(d, gpu, layout=layout)
    grad, loss, perm, before, after = a
    _check_sentinels(d, grad, perm, before, after)
    assert math.isnan(float(loss[1]))
    assert bool((grad[perm[1], :p] == 0.0).all()), "row 1's gradient"
    _check_accuracy(d["live"], grad, loss[[0, 2]], [perm[0], perm[2]], f"zero-length row {layout}")
    b = launch_grad(d, gpu, layout=layout, order=[0, 2])
    assert bool((b[0][perm[1]] == -7.0).all()), "the unlisted row was written"
    for k, r in enumerate([0, 2]):
        assert _row_bits_equal(d, a, b, r, k), r
