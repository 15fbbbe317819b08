"""--device-evaluation for GN-LeNet on the GPU: niidmix::gnlenet_eval_rows against the float64
restatement of tests/test_eval_gnlenet_host.py (which that file pins to the reference's own
log-probs), its layout, determinism and independence contracts, non-finite parameters, ties, and
DeviceEvaluator against the CPU loop.

Tolerances.  The network divides by a standard deviation, so there is no closed-form
condition-aware bound; per case e32 = max |z_fp32 - z64| over (job, sample, class), z_fp32 being
the same forward in torch fp32 on the CPU (the reference's arithmetic) and z64 the float64 forward.
The kernel's logits must be within 4 e32 of z64; pred equals the float64 argmax wherever the
float64 top-two gap exceeds 16 e32 (at most 1 % of a case's (job, sample) pairs may lie within it,
and the seeded cases have none); |loss_sum - loss64| <= 2 * 4 e32 * len (log-sum-exp and the
picked logit each move by at most the logits' error)."""
import math

import pytest
import torch
import torch.nn.functional as F

import test_eval_gnlenet_host as th

pytestmark = pytest.mark.gpu

TS = 2               # the kernel's sample tile (kGnTS)
M = 8                # samples per case
# (Cin, H, W, C): the minimum of every pooled map (7, 3, 1); non-square and odd; the reference's
# three shapes; one class; and a shape whose activations do not fit in LDS (the scratch-slot path)
SHAPES = [(1, 15, 15, 3), (3, 17, 15, 10), (1, 24, 24, 10), (1, 28, 28, 10), (3, 32, 32, 10),
          (1, 28, 28, 1), (2, 40, 36, 4)]
# jobs as (slab row, segment start, segment length): lengths 1, TS, TS + 1 and 0, a shared start
# (jobs 0 and 1), distinct ones, a row listed twice
JOBS = [(0, 0, TS + 1), (1, 0, TS + 1), (2, 3, TS), (0, 5, 1), (1, 2, 0), (2, 4, 2 * TS)]
N_ROWS = 3
_cache = {}


def _case(shape):
    """Inputs and the CPU references of a case, computed once: per slab row the float64 and fp32
    logits on all M samples."""
    if shape in _cache:
        return _cache[shape]
    cin, h, w, c = shape
    seed = 1000 + SHAPES.index(shape)
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    theta = torch.stack([torch.cat([q.detach().reshape(-1) for q in
                                    th.perturb(th.GNLeNet(cin, c, (h, w)), gen).parameters()])
                         for _ in range(N_ROWS)])
    x = torch.randn(M, cin, h, w, generator=gen)
    y = torch.randint(0, c, (M,), generator=gen)
    z64 = torch.stack([th.forward_logits(theta[r], x, c, torch.float64) for r in range(N_ROWS)])
    z32 = torch.stack([th.forward_logits(theta[r], x, c, torch.float32) for r in range(N_ROWS)])
    e32 = max(float((z32[r, s:s + n].double() - z64[r, s:s + n]).abs().max()) for r, s, n in JOBS if n)
    out = dict(shape=shape, theta=theta, x=x, y=y, z64=z64, z32=z32, e32=e32, p=theta.shape[1])
    _cache[shape] = out
    return out


def _launch(d, dev, jobs=JOBS, layout="vec", theta=None, with_pred=True, with_logits=True):
    """The op on `jobs` of a case.  Returns (loss_sum, correct, pred, logits, slab before, after);
    pred and logits carry sentinels (-7, -7.0) and two spare columns."""
    cin, h, w, c = d["shape"]
    p = d["p"]
    ld = (p + 3) // 4 * 4 if layout == "vec" else p + 1
    slab = torch.zeros(N_ROWS + 1, ld, device=dev)
    slab[:N_ROWS, :p] = (d["theta"] if theta is None else theta).to(dev)
    before = slab.clone()
    n = len(jobs)
    max_len = max(max(j[2] for j in jobs), 1)
    loss = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
    correct = torch.full((n,), -1, dtype=torch.int32, device=dev)
    pred = torch.full((n, max_len + 2), -7, dtype=torch.int32, device=dev)
    logits = torch.full((n, max_len + 2, c), -7.0, dtype=torch.float32, device=dev)
    col = lambda i: torch.tensor([j[i] for j in jobs], dtype=torch.int32, device=dev)  # noqa: E731
    torch.ops.niidmix.gnlenet_eval_rows(
        slab[:, :p], d["x"].reshape(M, -1).to(dev), d["y"].to(torch.int32).to(dev), col(0), col(1),
        col(2), max_len, loss, correct, pred[:, :max_len] if with_pred else None,
        logits if with_logits else None, cin, h, w, c)
    torch.cuda.synchronize()
    return loss.cpu(), correct.cpu(), pred.cpu(), logits.cpu(), before.cpu(), slab.cpu()


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(a, b):
    return all(torch.equal(_bits(u), _bits(v)) for u, v in zip(a[:4], b[:4]))


@pytest.mark.parametrize("layout", ["vec", "odd"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_float64(shape, layout, gpu):
    from niidmix import ops  # noqa: F401  (registers the op)
    d = _case(shape)
    c = shape[3]
    e32 = d["e32"]
    loss, correct, pred, logits, before, after = _launch(d, gpu, layout=layout)
    assert torch.equal(_bits(before), _bits(after)), "theta was written"
    worst, ambiguous, pairs = 0.0, 0, 0
    for i, (r, s, n) in enumerate(JOBS):
        assert bool((pred[i, n:] == -7).all()), "pred written past seg_len"
        assert bool((logits[i, n:] == -7.0).all()), "logits written past seg_len"
        if n == 0:
            assert float(loss[i]) == 0.0 and int(correct[i]) == 0
            continue
        z64, y = d["z64"][r, s:s + n], d["y"][s:s + n]
        worst = max(worst, float((logits[i, :n].double() - z64).abs().max()))
        pr = pred[i, :n].long()
        assert bool(((pr >= 0) & (pr < c)).all())
        if c > 1:
            top = z64.topk(2, dim=1).values
            amb = (top[:, 0] - top[:, 1]) <= 16 * e32
        else:
            amb = torch.zeros(n, dtype=torch.bool)
        ambiguous += int(amb.sum())
        pairs += n
        assert bool((pr[~amb] == z64.argmax(1)[~amb]).all()), "pred differs from the float64 argmax"
        for k in amb.nonzero().flatten().tolist():
            assert float(z64[k].max() - z64[k, pr[k]]) <= 16 * e32
        assert int(correct[i]) == int((pr == y).sum())
        nll = torch.logsumexp(z64, 1) - z64[torch.arange(n), y]
        assert abs(float(loss[i]) - float(nll.sum())) <= 2 * 4 * e32 * n
    print(f"{shape} {layout}: e32 {e32:.3g}  kernel max |z - z64| {worst:.3g}  ratio "
          f"{worst / e32 if e32 else 0.0:.3g}  max |z64| {float(d['z64'].abs().max()):.3g}")
    assert ambiguous <= 0.01 * pairs, "the case is ambiguous in float64: reseed it"
    assert worst <= 4 * e32, f"kernel logits off by {worst:.3g} = {worst / e32:.3g} e32"


@pytest.mark.parametrize("name", ["gn_lenet_mnist", "gn_lenet_cifar"])
def test_fixtures_through_the_kernel(name, gpu):
    """The reference's own model, samples and fp32 log-probs.  Logits within 4 e32 of float64;
    log_softmax moves by at most twice the logits' error, so the kernel's log-probs are within
    8 e32 + r of the fixture's, r being the fixture's own distance from float64."""
    from niidmix import ops  # noqa: F401
    g = th.load_fixture(name)
    cin, h, w, c = (int(v) for v in g["shape"])
    theta, x = torch.from_numpy(g["theta"]), torch.from_numpy(g["x"])
    y, ref = torch.from_numpy(g["y"]), torch.from_numpy(g["logprobs"]).double()
    z64 = th.forward_logits(theta, x, c, torch.float64)
    e32 = float((th.forward_logits(theta, x, c, torch.float32).double() - z64).abs().max())
    r = float((F.log_softmax(z64, 1) - ref).abs().max())
    dev = gpu
    slab = theta.reshape(1, -1).to(dev)
    loss = torch.empty(1, dtype=torch.float64, device=dev)
    correct = torch.empty(1, dtype=torch.int32, device=dev)
    pred = torch.empty((1, 4), dtype=torch.int32, device=dev)
    z = torch.empty((1, 4, c), dtype=torch.float32, device=dev)
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)  # noqa: E731
    torch.ops.niidmix.gnlenet_eval_rows(slab, x.reshape(4, -1).to(dev), y.to(torch.int32).to(dev),
                                        i32(0), i32(0), i32(4), 4, loss, correct, pred, z, cin, h, w, c)
    z = z[0].cpu().double()
    err = float((z - z64).abs().max())
    print(f"{name}: e32 {e32:.3g}  kernel {err:.3g}  ratio {err / e32:.3g}  fixture r {r:.3g}")
    assert err <= 4 * e32
    assert float((F.log_softmax(z, 1) - ref).abs().max()) <= 8 * e32 + r
    assert torch.equal(pred[0].cpu().long(), ref.argmax(1))
    assert int(correct[0]) == int((ref.argmax(1) == y).sum())
    assert abs(float(loss[0]) + float(ref[torch.arange(4), y].sum())) <= 4 * (8 * e32 + r)


@pytest.mark.parametrize("shape", [(3, 17, 15, 10), (1, 28, 28, 10), (2, 40, 36, 4)],
                         ids=lambda s: "x".join(map(str, s)))
def test_determinism_and_independence(shape, gpu):
    """Two calls give the same bits; a job alone gives the bits it gave among the others; the job
    list split over two calls gives the bits of one call; pred = logits = None changes nothing."""
    from niidmix import ops  # noqa: F401
    d = _case(shape)
    a = _launch(d, gpu)
    assert _same(a, _launch(d, gpu))
    for i, job in enumerate(JOBS):
        b = _launch(d, gpu, jobs=[job])
        n = job[2]
        assert torch.equal(_bits(b[0][0]), _bits(a[0][i])) and int(b[1][0]) == int(a[1][i]), i
        assert torch.equal(b[2][0, :n], a[2][i, :n]) and torch.equal(_bits(b[3][0, :n]), _bits(a[3][i, :n])), i
    for cut in (1, 4):
        lo, hi = _launch(d, gpu, jobs=JOBS[:cut]), _launch(d, gpu, jobs=JOBS[cut:])
        assert torch.equal(_bits(torch.cat([lo[0], hi[0]])), _bits(a[0]))
        assert torch.equal(torch.cat([lo[1], hi[1]]), a[1])
        for k, part in ((0, lo), (cut, hi)):
            for i in range(part[2].shape[0]):
                n = JOBS[k + i][2]
                assert torch.equal(part[2][i, :n], a[2][k + i, :n])
                assert torch.equal(_bits(part[3][i, :n]), _bits(a[3][k + i, :n]))
    b = _launch(d, gpu, with_pred=False, with_logits=False)
    assert torch.equal(_bits(b[0]), _bits(a[0])) and torch.equal(b[1], a[1])
    assert bool((b[2] == -7).all()) and bool((b[3] == -7.0).all())
    assert _same(a, _launch(d, gpu, layout="odd"))         # the leading dimension does not enter


def test_nan_stays_in_its_row(gpu):
    """A NaN in row 1's conv2.w: a NaN loss in the jobs that list row 1, the others bitwise as
    without it."""
    from niidmix import family, ops  # noqa: F401
    d = _case((1, 28, 28, 10))
    clean = _launch(d, gpu)
    theta = d["theta"].clone()
    off = family.gn_lenet_offsets(1, 10, 256)
    theta[1, off[4] + 12345] = float("nan")
    loss, correct, pred, logits, _, _ = _launch(d, gpu, theta=theta)
    for i, (r, s, n) in enumerate(JOBS):
        if r == 1 and n:
            assert math.isnan(float(loss[i])), i
        else:
            assert torch.equal(_bits(loss[i]), _bits(clean[0][i])) and int(correct[i]) == int(clean[1][i])
            assert torch.equal(pred[i], clean[2][i]) and torch.equal(_bits(logits[i]), _bits(clean[3][i]))


def test_ties_take_the_lowest_index(gpu):
    """Classes 1 and 3 with identical classifier rows and a bias that wins every sample."""
    from niidmix import family, ops  # noqa: F401
    d = _case((1, 28, 28, 10))
    off = family.gn_lenet_offsets(1, 10, 256)
    theta = d["theta"].clone()
    theta[0, off[12] + 3 * 256:off[12] + 4 * 256] = theta[0, off[12] + 256:off[12] + 2 * 256]
    theta[0, off[13] + 1] = theta[0, off[13] + 3] = 50.0
    loss, correct, pred, logits, _, _ = _launch(d, gpu, theta=theta, jobs=[(0, 0, M)])
    assert torch.equal(_bits(logits[0, :M, 1]), _bits(logits[0, :M, 3]))
    assert bool((pred[0, :M] == 1).all())
    assert int(correct[0]) == int((d["y"] == 1).sum())


# ------------------------------------------------------------------------------------------------
# DeviceEvaluator on 4 GN-LeNet nodes: train-sets of 70, 10, 130 and 33 samples, a 130-sample test set
N_NODES, N_TEST = 4, 130


def _params():
    return {"meta": {"log": "WARNING", "seed": 5}, "nodes": {"nb-nodes": N_NODES},
            "topology": {"name": "ring", "remove-clique-edges": 0}, "logger": {},
            "algorithm": {"learning-rate": 0.05, "learning-momentum": 0.0, "batch-size": 8,
                          "initial-averaging": False, "clique-gradient": False,
                          "unbiased-gradient": False, "device-evaluation": True}}


def _ring():
    w = torch.zeros(N_NODES, N_NODES)
    for i in range(N_NODES):
        for j in (i - 1, i, i + 1):
            w[i, j % N_NODES] = 1.0 / 3.0
    return {"edges": {i: [(i - 1) % N_NODES, (i + 1) % N_NODES] for i in range(N_NODES)}, "weights": w}


def _nodes(params, model=th.GNLeNet):
    from niidmix import d_sgd
    torch.manual_seed(77)
    gen = torch.Generator().manual_seed(78)
    x = torch.randn(300, 1, 28, 28, generator=gen)
    y = torch.randint(0, 10, (300,), generator=gen)
    nodes, a = [], 0
    for r, m in enumerate((70, 10, 130, 33)):
        mdl = th.perturb(model(), gen)
        nodes.append({"rank": r, "epoch": 0, "model": mdl, "optimizer": d_sgd.optimizer(mdl, params),
                      "train-set": [(x[i], int(y[i])) for i in range(a, a + m)]})
        a += m
    tests = [(x[i], int(y[i])) for i in range(300 - N_TEST, 300)]
    return nodes, tests


def _cpu_loop(model, samples, chunk):
    """The reference's loops in float64: (correct count, mean over chunks of each chunk's mean
    loss, e32 of this model on these samples, samples whose float64 top-two gap is within 16 e32)."""
    x = torch.stack([s[0] for s in samples])
    y = torch.tensor([s[1] for s in samples])
    theta = torch.cat([q.detach().reshape(-1) for q in model.parameters()])
    z64 = th.forward_logits(theta, x, 10, torch.float64)
    e32 = float((th.forward_logits(theta, x, 10, torch.float32).double() - z64).abs().max())
    nll = torch.logsumexp(z64, 1) - z64[torch.arange(len(samples)), y]
    parts = [nll[i:i + chunk] for i in range(0, len(samples), chunk)]
    top = z64.topk(2, dim=1).values
    return (int((z64.argmax(1) == y).sum()), sum(float(p.mean()) for p in parts) / len(parts), e32,
            int(((top[:, 0] - top[:, 1]) <= 16 * e32).sum()))


def _agrees(got, model, samples, chunk):
    correct, loss, e32, amb = _cpu_loop(model, samples, chunk)
    assert amb <= 0.01 * len(samples), "the float64 loop is ambiguous: reseed"
    # the same count, but for the samples whose float64 top-two gap is within 16 e32
    assert abs(got[0] * len(samples) - correct) <= amb + 1e-9, (got, correct, amb)
    assert abs(got[1] - loss) <= 2 * 4 * e32, (got, loss, e32)


def test_evaluator_against_the_cpu_loop(gpu):
    from niidmix import d_sgd, evaluate
    params = _params()
    nodes, tests = _nodes(params)
    d_sgd.init(nodes, _ring(), params)
    ev = evaluate.DeviceEvaluator(params).register_sets(test=tests)
    res = ev.accuracy(nodes, "test")
    assert ev.last_source == "stacked" and ev.last_calls == 1 and len(res) == N_NODES
    for nd, got in zip(nodes, res):
        _agrees(got, nd["model"], tests, N_TEST)
    train = ev.train_accuracy(nodes)
    assert ev.last_source == "stacked"
    for nd, got in zip(nodes, train):
        _agrees(got, nd["model"], nd["train-set"], 1000)
    assert ev.accuracy([nodes[2]["model"]], "test") == [res[2]]           # a subset: the same bits
    # the job list cut by a scratch budget of two jobs: more calls, the same bits
    from niidmix._lib import lib
    ev.scratch_budget = int(lib.niidmix_gnlenet_eval_rows_scratch_bytes(2, N_TEST, 1, 28, 28, 10))
    assert ev.accuracy(nodes, "test") == res and ev.last_calls == 2
    ev.scratch_budget = 8
    with pytest.raises(RuntimeError, match="device-evaluation"):
        ev.accuracy(nodes, "test")
    # a set the model does not take
    bad = evaluate.DeviceEvaluator(params).register_sets(test=[(s[0][:, :24, :20], s[1]) for s in tests])
    with pytest.raises(ValueError, match="device-evaluation"):
        bad.accuracy(nodes, "test")


def test_resident_slab_is_read_in_place(gpu):
    """After a resident round the parameters are read from its output slab on the device
    ("resident"); a write into a model makes the evaluator stack them again."""
    from niidmix import d_sgd, evaluate
    params = _params()
    nodes, tests = _nodes(params)
    topo = _ring()
    d_sgd.init(nodes, topo, params)
    d_sgd.average(nodes, topo, params)                     # one resident round
    eng = d_sgd._engines[id(nodes)]
    assert eng.resident is not None and eng.resident.fresh and len(eng.resident.parts) == 1
    ev = evaluate.DeviceEvaluator(params).register_sets(test=tests)
    res = ev.accuracy(nodes, "test")
    assert ev.last_source == "resident"
    d_sgd.synchronize()
    for nd, got in zip(nodes, res):
        _agrees(got, nd["model"], tests, N_TEST)
    assert ev.accuracy([nodes[3], nodes[1]], "test") == [res[3], res[1]] and ev.last_source == "resident"
    with torch.no_grad():
        nodes[1]["model"].classifier[0].bias.mul_(1.0)
    assert ev.accuracy(nodes, "test") == res and ev.last_source == "stacked"


def test_probe_refuses_another_group_count(gpu):
    """GroupNorm(4, .) has GN-LeNet's parameter shapes: only the forward probe can tell."""
    from niidmix import evaluate, family

    class FourGroups(th.GNLeNet):
        def __init__(self):
            super().__init__(groups=4)
    params = _params()
    nodes, tests = _nodes(params, FourGroups)
    assert family.gn_lenet_shape(nodes[0]["model"]) == (1, 10, 256)
    ev = evaluate.DeviceEvaluator(params).register_sets(test=tests)
    with pytest.raises(ValueError, match="device-evaluation.*GroupNorm"):
        ev.accuracy(nodes, "test")
