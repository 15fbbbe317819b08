"""--device-evaluation on the GPU: the evaluation kernel against float64, ties, its layout and
determinism contracts, non-finite parameters, DeviceEvaluator on the 16-node ring of
test_gpu_train, and the replaced Logger.state end to end."""
import json
import math
import os
import sys
import types

import pytest
import torch
import torch.nn.functional as F

import test_gpu_train as tg

pytestmark = pytest.mark.gpu

RTOL = 1e-5          # the project's fast-mode tolerance, on the condition-aware bound
TS = 64              # the kernel's sample tile (kEvTS): 64 and 256 are whole tiles, 257 = 4 TS + 1

# name: (jobs, samples, K, C, segment lengths or None (one shared segment), weight scale, layout)
#   layout 'vec': ld = P rounded up to 4 (float4 path where K allows); 'odd': ld = P + 1 (scalar)
CASES = {
    "784x10_shared_vec": (3, 257, 784, 10, None, 1.0, "vec"),
    "784x10_shared_odd_ld": (3, 257, 784, 10, None, 1.0, "odd"),
    "1023x1024": (2, 100, 1023, 1024, None, 1.0, "odd"),
    "33x7_segments": (4, 128, 33, 7, [64, 1, 63, 0], 1.0, "odd"),
    "5x3_one_sample": (1, 1, 5, 3, None, 1.0, "odd"),
    "4x1_one_class": (1, 5, 4, 1, None, 1.0, "vec"),
    "784x10_large_logits": (3, 257, 784, 10, None, 30.0, "vec"),
    "40x1024": (2, 32, 40, 1024, None, 1.0, "vec"),
}
_cache = {}


def _reference(x, y, w, b):
    """float64 logits z [M, C], A_s = max_c(|b_c| + sum_k |x_sk| |W_ck|), the top-two gap and
    nll_s of one job (x [M, K], w [C, K], b [C] fp32 values)."""
    xd, wd, bd = x.double(), w.double(), b.double()
    z = xd @ wd.t() + bd
    a = (xd.abs() @ wd.abs().t() + bd.abs()).max(1).values
    if z.shape[1] > 1:
        top = z.topk(2, dim=1).values
        gap = top[:, 0] - top[:, 1]
    else:
        gap = torch.full((z.shape[0],), float("inf"), dtype=torch.float64)
    nll = torch.logsumexp(z, 1) - z[torch.arange(z.shape[0]), y]
    return z, a, gap, nll


def _case(name):
    """Inputs and per-job float64 / fp32 torch CPU references of a case, computed once."""
    if name in _cache:
        return _cache[name]
    n, m, k, c, lens, scale, layout = CASES[name]
    gen = torch.Generator().manual_seed(list(CASES).index(name))
    x = torch.randn(m, k, generator=gen, dtype=torch.float64).float()
    y = torch.randint(0, c, (m,), generator=gen)
    w = (torch.randn(n, c, k, generator=gen, dtype=torch.float64) / math.sqrt(k) * scale).float()
    b = (0.1 * torch.randn(n, c, generator=gen, dtype=torch.float64)).float()
    if lens is None:
        starts, lens = [0] * n, [m] * n
    else:
        starts = [0, 64, 65, 128][:n]
    refs, l32 = [], []
    for i in range(n):
        xi, yi = x[starts[i]:starts[i] + lens[i]], y[starts[i]:starts[i] + lens[i]]
        refs.append(_reference(xi, yi, w[i], b[i]))
        l32.append(float(F.nll_loss(F.log_softmax(F.linear(xi, w[i], b[i]), 1), yi, reduction="sum"))
                   if lens[i] else 0.0)
    out = dict(n=n, m=m, k=k, c=c, starts=starts, lens=lens, layout=layout, x=x, y=y,
               theta=torch.cat([w.reshape(n, -1), b], 1), refs=refs, l32=l32)
    _cache[name] = out
    return out


def _ld(p, layout):
    return (p + 3) // 4 * 4 if layout == "vec" else p + 1


def _launch(d, dev, jobs=None, rows=None, n_slab=None, theta=None, with_pred=True, sentinel=-7):
    """The op on jobs `jobs` of a case (default all), job j reading slab row rows[j].  Returns
    (loss_sum, correct, pred or None, theta slab before, theta slab after)."""
    n, k, c = d["n"], d["k"], d["c"]
    p = c * k + c
    jobs = list(range(n)) if jobs is None else jobs
    rows = jobs if rows is None else rows
    n_slab = n_slab or max(rows) + 1
    th = torch.zeros(n_slab, _ld(p, d["layout"]), device=dev)
    src = d["theta"] if theta is None else theta
    for j, r in zip(jobs, rows):
        th[r, :p] = src[j].to(dev)
    before = th.clone()
    lens = [d["lens"][j] for j in jobs]
    max_len = max(max(lens), 1)
    loss = torch.full((len(jobs),), -1.0, dtype=torch.float64, device=dev)
    correct = torch.full((len(jobs),), -1, dtype=torch.int32, device=dev)
    pred = torch.full((len(jobs), max_len + 2), sentinel, dtype=torch.int32, device=dev) if with_pred else None
    torch.ops.niidmix.linear_eval_rows(
        th[:, :p], d["x"].to(dev), d["y"].to(torch.int32).to(dev),
        torch.tensor(rows, dtype=torch.int32, device=dev),
        torch.tensor([d["starts"][j] for j in jobs], dtype=torch.int32, device=dev),
        torch.tensor(lens, dtype=torch.int32, device=dev), max_len, loss, correct,
        pred[:, :max_len] if with_pred else None, k, c)
    torch.cuda.synchronize()
    return loss.cpu(), correct.cpu(), pred.cpu() if with_pred else None, before.cpu(), th.cpu()


def _check_job(pred, loss_sum, correct, ref, y):
    """The issue's checks of one job; returns the loss error over its bound (0 when both are 0)."""
    z, a, gap, nll = ref
    m = z.shape[0]
    amb = gap <= 2e-5 * a
    assert float(amb.double().mean()) <= 0.01 if m else True, "the case is ambiguous in float64"
    am = z.argmax(1)
    pred = pred[:m].long()
    assert bool(((pred >= 0) & (pred < z.shape[1])).all())
    assert bool((pred[~amb] == am[~amb]).all()), "pred differs from the float64 argmax"
    for s in amb.nonzero().flatten().tolist():
        assert float(z[s].max() - z[s, pred[s]]) <= 2e-5 * float(a[s])
    assert int(correct) == int((pred == y).sum())
    err, bound = abs(float(loss_sum) - float(nll.sum())), RTOL * float((2 * a).sum())
    assert err <= bound, f"loss_sum off by {err:.3g}, bound {bound:.3g}"
    return err / bound * RTOL if bound else 0.0


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_float64(name, gpu):
    """pred equals the float64 argmax wherever the float64 top-two gap exceeds 2e-5 A_s (and is
    within that gap of the maximum elsewhere; at most 1 % of a case may be such), correct counts
    pred == y exactly, |loss_sum - loss64| <= 1e-5 sum_s 2 A_s."""
    from niidmix import ops  # noqa: F401  (registers the op)
    d = _case(name)
    loss, correct, pred, before, after = _launch(d, gpu)
    assert torch.equal(before.view(torch.int32), after.view(torch.int32))
    worst, worst32 = 0.0, 0.0
    for i in range(d["n"]):
        yi = d["y"][d["starts"][i]:d["starts"][i] + d["lens"][i]]
        worst = max(worst, _check_job(pred[i], loss[i], correct[i], d["refs"][i], yi))
        bound = float((2 * d["refs"][i][1]).sum())
        if bound:
            worst32 = max(worst32, abs(d["l32"][i] - float(d["refs"][i][3].sum())) / bound)
        assert bool((pred[i, d["lens"][i]:] == -7).all()), "pred written past seg_len"
    print(f"{name}: worst |loss_sum - loss64| / sum 2A  kernel {worst:.3g}  torch fp32 {worst32:.3g}")
    assert worst32 <= RTOL, "torch fp32 outside the bound: the inputs are wrong for this test"
    if name == "4x1_one_class":
        assert float(loss[0]) == 0.0 and bool((pred[0, :5] == 0).all())
    if name == "33x7_segments":
        assert float(loss[3]) == 0.0 and int(correct[3]) == 0            # a job of length 0


def test_ties(gpu):
    """Two classes with identical weights and bias that win every sample: the lower index.
    All-zero parameters: class 0, and every nll_s is fp32 log C -- A_s is 0 there, so what is
    left is the fp32 rounding of nll_s itself, taken as 2 ulp (2^-22 relative) per sample."""
    from niidmix import ops  # noqa: F401
    m, k, c = 130, 16, 5
    gen = torch.Generator().manual_seed(77)
    x = torch.rand(m, k, generator=gen) + 0.1
    w = -torch.ones(2, c, k)
    w[0, 1] = w[0, 3] = 1.0
    b = torch.zeros(2, c)
    w[1], b[1] = 0.0, 0.0
    d = dict(n=2, m=m, k=k, c=c, starts=[0, 0], lens=[m, m], layout="vec", x=x,
             y=torch.full((m,), 3), theta=torch.cat([w.reshape(2, -1), b], 1))
    loss, correct, pred, _, _ = _launch(d, gpu)
    assert bool((pred[0, :m] == 1).all()) and int(correct[0]) == 0
    assert bool((pred[1, :m] == 0).all()) and int(correct[1]) == 0
    assert abs(float(loss[1]) - m * math.log(c)) <= m * math.log(c) * 2.0 ** -22


def test_layout_and_determinism(gpu):
    """Jobs list rows [5, 0, 3, 5] of an 8-row slab, out of order, row 5 twice: theta is bitwise
    unchanged, the sentinel survives in pred at and past seg_len, the twin jobs agree bitwise, two
    calls agree bitwise, each job run alone gives the bits it gave in the batch, and pred = None
    gives the same loss_sum / correct."""
    from niidmix import ops  # noqa: F401
    for name in ("33x7_segments", "784x10_shared_vec", "40x1024"):
        d = _case(name)
        jobs = [2, 0, 1, 2] if d["n"] >= 3 else [1, 0, 1, 1]
        rows = [5, 0, 3, 5]
        a = _launch(d, gpu, jobs=jobs, rows=rows, n_slab=8)
        loss, correct, pred, before, after = a
        assert torch.equal(before.view(torch.int32), after.view(torch.int32)), name
        for i, j in enumerate(jobs):
            assert bool((pred[i, d["lens"][j]:] == -7).all()), name
            assert not bool((pred[i, :d["lens"][j]] == -7).any()), name
        assert torch.equal(loss[0].view(torch.int64), loss[3].view(torch.int64))
        assert int(correct[0]) == int(correct[3]) and torch.equal(pred[0], pred[3]), name
        b = _launch(d, gpu, jobs=jobs, rows=rows, n_slab=8)
        assert all(torch.equal(u, v) for u, v in zip(a[:3], b[:3])), name
        for i in range(3):
            lo, co, pr, _, _ = _launch(d, gpu, jobs=[jobs[i]], rows=[rows[i]], n_slab=8)
            ln = d["lens"][jobs[i]]
            assert torch.equal(lo[0].view(torch.int64), loss[i].view(torch.int64)), (name, i)
            assert int(co[0]) == int(correct[i]) and torch.equal(pr[0, :ln], pred[i, :ln]), (name, i)
        lo, co, pr, _, _ = _launch(d, gpu, jobs=jobs, rows=rows, n_slab=8, with_pred=False)
        assert pr is None and torch.equal(lo.view(torch.int64), loss.view(torch.int64))
        assert torch.equal(co, correct), name


def test_non_finite_stays_in_its_job(gpu):
    """An inf weight in job 1's row: jobs 0 and 2 give the bits of a call without it.  A NaN
    weight: that class's logit is NaN on every sample and pred is torch.argmax of the fp32 CPU
    logits (the first NaN)."""
    from niidmix import ops  # noqa: F401
    d = _case("784x10_shared_vec")
    clean = _launch(d, gpu)
    theta = d["theta"].clone()
    theta[1, 3 * d["k"] + 5] = float("inf")
    loss, correct, pred, _, _ = _launch(d, gpu, theta=theta)
    for i in (0, 2):
        assert torch.equal(loss[i].view(torch.int64), clean[0][i].view(torch.int64))
        assert int(correct[i]) == int(clean[1][i]) and torch.equal(pred[i], clean[2][i])
    assert not math.isfinite(float(loss[1]))
    theta = d["theta"].clone()
    theta[0, 6 * d["k"] + 2] = float("nan")
    theta[0, 2 * d["k"] + 9] = float("nan")
    loss, correct, pred, _, _ = _launch(d, gpu, theta=theta)
    k, c = d["k"], d["c"]
    z32 = F.linear(d["x"], theta[0, :c * k].view(c, k), theta[0, c * k:])
    assert torch.equal(pred[0, :d["m"]].long(), z32.argmax(1)) and bool((pred[0, :d["m"]] == 2).all())
    assert math.isnan(float(loss[0]))
    for i in (1, 2):
        assert torch.equal(loss[i].view(torch.int64), clean[0][i].view(torch.int64))


# ------------------------------------------------------------------------------------------------
# DeviceEvaluator on the 16-node ring of test_gpu_train: Linear(784, 10), batch 25; train-sets of
# 40 samples, node 5 with 1003 (two chunks); a 300-sample test set
N, K, C = tg.N, tg.K, tg.C
BIG, N_TEST = 5, 300


def _test_set():
    g = torch.Generator().manual_seed(314)
    x = torch.rand(N_TEST, 1, 28, 28, generator=g) * (torch.rand(N_TEST, 1, 28, 28, generator=g) < 0.05)
    y = torch.randint(0, C, (N_TEST,), generator=g)
    return [(x[i], int(y[i])) for i in range(N_TEST)]


def _setup(device_training, **logger_params):
    from niidmix import d_sgd
    torch.manual_seed(2024)
    lp = {"accuracy-logging-interval": 0, "accuracy-logging-interval-steps": 0,
          "log-consensus-distance": False}
    lp.update(logger_params)
    params = {"meta": {"log": "WARNING", "seed": 2024}, "model": {"input-size": K},
              "nodes": {"nb-nodes": N}, "topology": {"name": "ring", "remove-clique-edges": 0},
              "logger": lp,
              "algorithm": {"learning-rate": tg.LR, "learning-momentum": 0.0, "batch-size": tg.B,
                            "initial-averaging": False, "clique-gradient": False,
                            "unbiased-gradient": False, "deferred-writeback": False,
                            "mixing-mode": "exact", "device-evaluation": True}}
    if device_training:
        params["algorithm"]["device-training"] = True
    x, y = tg._dataset()
    nodes = []
    for r in range(N):
        idx = [(r * 40 + j) % (N * tg.S) for j in range(1003 if r == BIG else 40)]
        mdl = tg.Net()
        nodes.append({"rank": r, "epoch": 0, "train-set": [(x[i], int(y[i])) for i in idx],
                      "model": mdl, "optimizer": d_sgd.optimizer(mdl, params)})
    state, _, _ = d_sgd.init(nodes, tg._ring(), params)
    return params, nodes, state


def _restate(model, samples, chunk):
    """An independent float64 restatement on the CPU: (accuracy, loss, loss bound, ambiguous
    samples) with the loss the mean over chunks of `chunk` samples of each chunk's mean."""
    x = torch.stack([s[0] for s in samples]).view(len(samples), -1)
    y = torch.tensor([s[1] for s in samples])
    z, a, gap, nll = _reference(x, y, model.fc.weight.detach(), model.fc.bias.detach())
    parts = [slice(i, min(i + chunk, len(samples))) for i in range(0, len(samples), chunk)]
    loss = sum(float(nll[p].mean()) for p in parts) / len(parts)
    bound = sum(RTOL * float((2 * a[p]).mean()) for p in parts) / len(parts)
    return float((z.argmax(1) == y).double().mean()), loss, bound, int((gap <= 2e-5 * a).sum())


def _agrees(got, model, samples, chunk):
    acc, loss, bound, amb = _restate(model, samples, chunk)
    assert amb <= 0.01 * len(samples), "the float64 restatement is ambiguous"
    # equal, but for the samples whose float64 top-two gap is within 2e-5 A_s (none in practice)
    assert abs(got[0] - acc) <= (amb + 1e-9) / len(samples), (got, acc, amb)
    assert abs(got[1] - loss) <= bound, (got, loss, bound)


@pytest.mark.parametrize("device_training", [True, False])
def test_evaluator_on_the_ring(device_training, gpu):
    from niidmix import d_sgd, evaluate
    params, nodes, state = _setup(device_training)
    for _ in range(3):
        state, _, _, _ = d_sgd.next_step(state, params, None)
    d_sgd.synchronize()
    tests = _test_set()
    ev = evaluate.DeviceEvaluator(params).register_sets(test=tests)
    tr = d_sgd.device_trainer([nd["model"] for nd in nodes])
    uploads = tr[0].param_uploads if device_training else None
    assert (tr is not None) == device_training
    source = "trainer" if device_training else "stacked"
    res = ev.train_accuracy(nodes)
    assert ev.last_source == source and len(res) == N
    for nd, got in zip(nodes, res):
        _agrees(got, nd["model"], nd["train-set"], 1000)
    res = ev.accuracy(nodes, "test")
    assert ev.last_source == source
    for nd, got in zip(nodes, res):
        _agrees(got, nd["model"], tests, N_TEST)
    assert ev.accuracy([nodes[2]], "test") == [res[2]]                   # a subset: the same bits
    assert evaluate.DeviceEvaluator(params).register_sets(valid=[]).accuracy(nodes[:2], "valid") == \
        [(0.0, 0.0)] * 2
    if not device_training:
        return
    assert tr[0].param_uploads == uploads
    # a write into one model between rounds is seen (its version counter moves)
    with torch.no_grad():
        nodes[3]["model"].fc.weight.mul_(-1.0)
    after = ev.accuracy(nodes, "test")
    assert ev.last_source == "stacked" and tr[0].param_uploads == uploads
    _agrees(after[3], nodes[3]["model"], tests, N_TEST)
    assert after[3] != res[3] and after[:3] == res[:3] and after[4:] == res[4:]
    state, _, _, _ = d_sgd.next_step(state, params, None)
    assert tr[0].param_uploads == uploads + 1
    ev.accuracy(nodes, "test")
    assert ev.last_source == "trainer"


def test_non_linear_model_is_refused(gpu):
    from niidmix import evaluate

    class Scaled(tg.Net):
        def forward(self, x, params):
            return F.log_softmax(2.0 * self.fc(x.view(-1, K)), dim=1)
    ev = evaluate.DeviceEvaluator({}).register_sets(test=_test_set())
    with pytest.raises(ValueError, match="device-evaluation"):
        ev.accuracy([Scaled()], "test")


def test_logger_state_end_to_end(gpu, monkeypatch, tmp_path):
    """A stand-in Logger with the flag on: one state(nodes, ..) call writes the per-node and
    global event lines with exactly the schema's keys and the evaluator's values."""
    from niidmix import evaluate, logger as nl
    lg = types.ModuleType("simulate.logger")

    class Logger:
        def __init__(self, params, rundir):
            self.params, self.rundir = params, rundir
            self.running_loss = [0.0] * N
            self.running_loss_count = [0] * N
            self.global_events = os.path.join(rundir, "events", "global.jsonlines")

        def state(self, nodes, state):
            raise AssertionError("the reference's ssh version")

        def log_consensus_distance(self, state):
            raise AssertionError("reference CPU version")
    lg.Logger = Logger
    monkeypatch.setitem(sys.modules, "simulate.logger", lg)
    monkeypatch.setattr(evaluate, "_default", None)
    params, nodes, state = _setup(False, **{"log-global-model-accuracy": True,
                                            "skip-full-training": True})
    assert Logger.state is nl.device_state
    (tmp_path / "events").mkdir()
    for nd in nodes:
        nd["event-file"] = str(tmp_path / "events" / f"{nd['rank']}.jsonlines")
    tests = _test_set()
    full = [s for nd in nodes[:3] for s in nd["train-set"]]
    evaluate.register_sets(test=tests, valid=tests[:100], full_train=full, params=params)
    logger = Logger(params, str(tmp_path))
    logger.running_loss[1], logger.running_loss_count[1] = 3.0, 2
    logged = nodes[:2]
    logger.state(logged, {"step": 4})
    ev = evaluate.default(params)
    want_train = ev.train_accuracy(logged)
    want = {name: ev.accuracy(logged, name) for name in ("test", "valid")}
    center = nl.average([nd["model"] for nd in logged])
    want_global = [ev.accuracy([center], name)[0] for name in ("full-train", "test", "valid")]
    keys = ["type", "data", "rank", "epoch", "step", "loss", "accuracy", "timestamp"]
    for i, nd in enumerate(logged):
        lines = [json.loads(ln) for ln in open(nd["event-file"])]
        assert [e["data"] for e in lines] == ["train", "test", "valid"]
        assert list(lines[0]) == keys[:6] + ["running_loss"] + keys[6:]
        assert all(list(e) == keys for e in lines[1:])
        assert all(e["type"] == "accuracy" and e["rank"] == nd["rank"] and e["step"] == 4
                   and e["epoch"] == 0 for e in lines)
        assert (lines[0]["accuracy"], lines[0]["loss"]) == want_train[i]
        assert lines[0]["running_loss"] == (1.5 if i == 1 else 0.0)
        for e in lines[1:]:
            assert (e["accuracy"], e["loss"]) == want[e["data"]][i]
    lines = [json.loads(ln) for ln in open(logger.global_events)]
    assert [e["data"] for e in lines] == ["train", "test", "valid"]
    assert all(list(e) == ["type", "data", "epoch", "step", "loss", "accuracy", "timestamp"]
               for e in lines)
    assert [(e["accuracy"], e["loss"]) for e in lines] == want_global
    assert sorted(os.listdir(tmp_path)) == ["events"]
