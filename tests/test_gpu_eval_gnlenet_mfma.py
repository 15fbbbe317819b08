"""niidmix::gnlenet_eval_rows_mfma on the GPU against the float64 forward under the bounds of
tests/test_gpu_eval_gnlenet.py, which reasons them (e32 = torch's fp32 CPU error on the case); its
bitwise contracts, a NaN parameter, its shape limit, DeviceEvaluator under --device-evaluation-mfma."""
import functools
import math

import pytest
import torch

import test_eval_gnlenet_host as th
import test_gpu_eval_gnlenet as tg

pytestmark = pytest.mark.gpu

M, N_ROWS = 12, 3
# (Cin, H, W, C): pooled maps of 7 / 3 / 1 (conv3's M nearly all padding); non-square and odd; the
# reference's shapes at tile 4 and 2; one class.  Jobs (slab row, start, length): lengths 2 T + 1,
# T + 1, T, 1 and 0 at the kernel's tile T, jobs 0 and 1 share a start, row 0 is listed twice.
SHAPES = [(1, 15, 15, 3), (3, 17, 15, 10), (1, 28, 28, 10), (3, 32, 32, 10), (1, 28, 28, 1)]
OVER = (2, 44, 44, 10)           # no tile of 2 samples fits in LDS


@functools.lru_cache(None)
def _case(shape):
    """tg._case on this file's shapes and jobs: inputs and the float64 / fp32 CPU logits, once."""
    from niidmix import ops
    cin, h, w, c = shape
    seed = 2000 + SHAPES.index(shape)
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    theta = torch.stack([torch.cat([q.detach().reshape(-1) for q in
                                    th.perturb(th.GNLeNet(cin, c, (h, w)), gen).parameters()])
                         for _ in range(N_ROWS)])
    x = torch.randn(M, cin, h, w, generator=gen)
    y = torch.randint(0, c, (M,), generator=gen)
    z64 = torch.stack([th.forward_logits(theta[r], x, c, torch.float64) for r in range(N_ROWS)])
    z32 = torch.stack([th.forward_logits(theta[r], x, c, torch.float32) for r in range(N_ROWS)])
    t = ops.gn_mfma_tile(h, w)
    jobs = [(0, 0, 2 * t + 1), (1, 0, t + 1), (2, 3, t), (0, 5, 1), (1, 2, 0)]
    e32 = max(float((z32[r, s:s + n].double() - z64[r, s:s + n]).abs().max()) for r, s, n in jobs if n)
    return dict(shape=shape, theta=theta, x=x, y=y, z64=z64, e32=e32, p=theta.shape[1], jobs=jobs)


def _launch(d, dev, jobs=None, layout="vec", theta=None, outputs=True):
    """(loss_sum, correct, pred, logits, slab before, after); sentinels -7 in pred and logits."""
    cin, h, w, c = d["shape"]
    jobs, p = d["jobs"] if jobs is None else jobs, d["p"]
    ld = (p + 3) // 4 * 4 if layout == "vec" else p + 1
    slab = torch.zeros(N_ROWS + 1, ld, device=dev)
    slab[:N_ROWS, :p] = (d["theta"] if theta is None else theta).to(dev)
    before = slab.clone()
    n, max_len = len(jobs), max(max(j[2] for j in jobs), 1)
    loss = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
    correct = torch.full((n,), -1, dtype=torch.int32, device=dev)
    pred = torch.full((n, max_len + 2), -7, dtype=torch.int32, device=dev)
    logits = torch.full((n, max_len + 2, c), -7.0, dtype=torch.float32, device=dev)
    col = lambda i: torch.tensor([j[i] for j in jobs], dtype=torch.int32, device=dev)  # noqa: E731
    torch.ops.niidmix.gnlenet_eval_rows_mfma(
        slab[:, :p], d["x"].reshape(M, -1).to(dev), d["y"].to(torch.int32).to(dev), col(0), col(1),
        col(2), max_len, loss, correct, pred[:, :max_len] if outputs else None,
        logits if outputs else None, cin, h, w, c)
    torch.cuda.synchronize()
    return loss.cpu(), correct.cpu(), pred.cpu(), logits.cpu(), before.cpu(), slab.cpu()


def _same_job(a, i, b, k, n):
    return (torch.equal(tg._bits(a[0][i]), tg._bits(b[0][k])) and int(a[1][i]) == int(b[1][k]) and
            torch.equal(a[2][i, :n], b[2][k, :n]) and torch.equal(tg._bits(a[3][i, :n]), tg._bits(b[3][k, :n])))


@pytest.mark.parametrize("layout", ["vec", "odd"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_float64(shape, layout, gpu):
    from niidmix import ops  # noqa: F401  (registers the op)
    d = _case(shape)
    c, e32 = shape[3], d["e32"]
    loss, correct, pred, logits, before, after = _launch(d, gpu, layout=layout)
    assert torch.equal(tg._bits(before), tg._bits(after)), "theta was written"
    ambiguous, pairs = 0, 0
    assert float(loss[4]) == 0.0 and int(correct[4]) == 0                 # the job of length 0
    for i, (r, s, n) in enumerate(d["jobs"]):
        assert bool((pred[i, n:] == -7).all()) and bool((logits[i, n:] == -7.0).all()), "past seg_len"
        if n == 0:
            continue
        z64, y = d["z64"][r, s:s + n], d["y"][s:s + n]
        worst = float((logits[i, :n].double() - z64).abs().max())
        assert worst <= 4 * e32, f"kernel logits off by {worst:.3g} = {worst / e32:.3g} e32"
        pr = pred[i, :n].long()
        top = z64.topk(2, dim=1).values if c > 1 else torch.tensor([[1.0, 0.0]]).expand(n, 2)
        amb = (top[:, 0] - top[:, 1]) <= 16 * e32
        ambiguous += int(amb.sum())
        pairs += n
        assert bool((pr[~amb] == z64.argmax(1)[~amb]).all()), "pred differs from the float64 argmax"
        assert int(correct[i]) == int((pr == y).sum())
        nll = torch.logsumexp(z64, 1) - z64[torch.arange(n), y]
        assert abs(float(loss[i]) - float(nll.sum())) <= 2 * 4 * e32 * n
    assert ambiguous <= 0.01 * pairs, "the case is ambiguous in float64: reseed it"


@pytest.mark.parametrize("shape", [(3, 17, 15, 10), (1, 28, 28, 10)], ids=lambda s: "x".join(map(str, s)))
def test_determinism_independence_and_tile_position(shape, gpu):
    """Equal bits: repeated, a job alone, the list cut twice, no pred / logits, any tile position."""
    d = _case(shape)
    jobs, t = d["jobs"], d["jobs"][2][2]
    a, b = _launch(d, gpu), _launch(d, gpu)
    assert all(torch.equal(tg._bits(u), tg._bits(v)) for u, v in zip(a[:4], b[:4]))
    for i, job in enumerate(jobs):
        assert _same_job(_launch(d, gpu, jobs=[job]), 0, a, i, job[2]), i
    for cut in (1, 3):
        for k, part in ((0, _launch(d, gpu, jobs=jobs[:cut])), (cut, _launch(d, gpu, jobs=jobs[cut:]))):
            for i in range(part[0].shape[0]):
                assert _same_job(part, i, a, k + i, jobs[k + i][2]), (cut, k + i)
    b = _launch(d, gpu, outputs=False)
    assert torch.equal(tg._bits(b[0]), tg._bits(a[0])) and torch.equal(b[1], a[1])
    assert bool((b[2] == -7).all()) and bool((b[3] == -7.0).all())
    single = _launch(d, gpu, jobs=[(0, s, 1) for s in range(2 * t + 1)])
    for s in range(2 * t + 1):
        assert torch.equal(tg._bits(single[3][s, 0]), tg._bits(a[3][0, s])), s


def test_nan_stays_in_its_row(gpu):
    """A NaN in row 1's conv2.w: a NaN loss exactly in the jobs that list row 1."""
    from niidmix import family
    d = _case((1, 28, 28, 10))
    clean = _launch(d, gpu)
    theta = d["theta"].clone()
    theta[1, family.gn_lenet_offsets(1, 10, 256)[4] + 12345] = float("nan")
    got = _launch(d, gpu, theta=theta)
    for i, (r, s, n) in enumerate(d["jobs"]):
        assert math.isnan(float(got[0][i])) if r == 1 and n else _same_job(got, i, clean, i, n + 2), i


def test_shape_beyond_the_lds_limit_is_unsupported(gpu):
    from niidmix import _lib, ops
    cin, h, w, c = OVER
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=gpu)  # noqa: E731
    with pytest.raises(_lib.NiidmixError, match=f"niidmix error {_lib.EUNSUPPORTED}.*matrix-core"):
        torch.ops.niidmix.gnlenet_eval_rows_mfma(
            torch.zeros(1, ops.gnlenet_sizes(*OVER)[1], device=gpu), torch.zeros(2, cin * h * w, device=gpu), i32(0).repeat(2),
            i32(0), i32(0), i32(2), 2, torch.empty(1, dtype=torch.float64, device=gpu), i32(0), None,
            None, cin, h, w, c)


@pytest.mark.parametrize("shape,kernel", [((1, 28, 28, 10), "k_gnl_eval_mfma"), (OVER, "k_gnl_eval")])
def test_evaluator_takes_the_kernel_the_rule_names(shape, kernel, gpu):
    """DeviceEvaluator under both flags on 4 nodes against the float64 CPU loop (tg._agrees)."""
    from niidmix import d_sgd, evaluate
    cin, h, w, c = shape
    params = tg._params()
    params["algorithm"]["device-evaluation-mfma"] = True
    torch.manual_seed(91)
    gen = torch.Generator().manual_seed(92)
    x = torch.randn(43, cin, h, w, generator=gen)
    y = torch.randint(0, c, (43,), generator=gen)
    tests = [(x[i], int(y[i])) for i in range(23, 43)]
    mdls = [th.perturb(th.GNLeNet(cin, c, (h, w)), gen) for _ in range(4)]
    nodes = [{"rank": r, "epoch": 0, "model": m, "optimizer": d_sgd.optimizer(m, params),
              "train-set": tests} for r, m in enumerate(mdls)]
    d_sgd.init(nodes, tg._ring(), params)
    ev = evaluate.DeviceEvaluator(params).register_sets(test=tests)
    for nd, got in zip(nodes, ev.accuracy(nodes, "test")):
        tg._agrees(got, nd["model"], tests, len(tests))
    assert ev.last_kernel == kernel and ev.last_source == "stacked"
