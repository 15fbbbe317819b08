"""niidmix::sample_step_mean_update (the 'sample' round's optimizer step, average and broadcast in one
launch) against (a) the three ops it restates, run in sequence on the same inputs, and (b) the
reference's CPU arithmetic: torch.optim.SGD.step on the active rows (a first step is a fresh
optimizer), setup.model.average with [1/k]*k in the sample's order, update_models of every row
(_ref_sample_round in tests/test_gpu_dropin.py shows the latter two).  Bit for bit, NaNs by
position."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LR, MOM, SENT = 0.1, 0.9, 12345.0


def _same_bits(a, b):
    a, b = a.cpu(), b.cpu()
    nan = torch.isnan(b)
    return torch.equal(torch.isnan(a), nan) and \
        torch.equal(a[~nan].view(torch.int32), b[~nan].view(torch.int32))


def _cpu_round(x, g, buf, active, first, momentum, lr=LR):
    """(y, buf') of the reference's round on CPU tensors [N, P]."""
    n, k = x.shape[0], len(active)
    stepped, new_buf = {}, buf.clone()
    for j, r in enumerate(active):
        q = torch.nn.Parameter(x[r].clone())
        q.grad = g[r].clone()
        opt = torch.optim.SGD([q], lr=lr, momentum=momentum)
        if momentum and not first[j]:
            opt.state[q]["momentum_buffer"] = buf[r].clone()
        opt.step()
        stepped[r] = q.detach()
        if momentum:
            new_buf[r] = opt.state[q]["momentum_buffer"]
    with torch.no_grad():
        w = [1 / k for _ in active]
        center = stepped[active[0]].clone()
        center.mul_(0)
        for r, wi in zip(active, w):
            center.add_(wi * stepped[r])
        y = torch.stack([stepped.get(i, x[i]).clone() for i in range(n)])
        for i in range(n):
            y[i].mul_(0.)
            y[i].add_(center)
    return y, new_buf


def _padded(t, ld, dev):
    full = torch.full((t.shape[0], ld), SENT, dtype=torch.float32)
    full[:, :t.shape[1]] = t
    full = full.to(dev)
    return full, full[:, :t.shape[1]]


def _device_round(dev, x, g, buf, active, first, momentum, ld, fused):
    """The fused op, or the three ops in sequence, on padded device copies; returns the full
    [N, ld] slabs (x, y, g, buf) after the call."""
    from niidmix import ops
    p = x.shape[1]
    xf, xv = _padded(x, ld, dev)
    yf, yv = _padded(torch.full_like(x, SENT), ld, dev)
    gf, gv = _padded(g, ld, dev)
    bf, bv = _padded(buf, ld, dev)
    act = torch.tensor(active, dtype=torch.int32, device=dev)
    fl = torch.tensor([int(f) for f in first], dtype=torch.int32, device=dev)
    k = len(active)
    if fused:
        ops.sample_step_mean_update(xv, yv, gv, bv if momentum else None, act, fl if momentum else None,
                                    -LR, momentum)
    else:
        if momentum:
            for want in (True, False):
                rows = torch.tensor([r for r, f in zip(active, first) if bool(f) == want],
                                    dtype=torch.int32, device=dev)
                if rows.numel():
                    ops.sgd_momentum_step_rows(xv, gv, bv, rows, -LR, momentum, want)
        else:
            ops.sgd_step_rows(xv, gv, act, -LR)
        avg = torch.empty((1, p), dtype=torch.float32, device=dev)
        ops.mix_csr(xv, torch.tensor([0, k], dtype=torch.int64, device=dev), act,
                    torch.full((k,), float(np.float32(1.0 / k)), dtype=torch.float32, device=dev), avg,
                    ops.EXACT | ops.AVERAGE_ONLY)
        ops.update_rows(xv, avg[0], yv)
    torch.cuda.synchronize()
    return xf.cpu(), yf.cpu(), gf.cpu(), bf.cpu()


def _check(dev, x, g, buf, active, first, momentum, ld):
    p, n = x.shape[1], x.shape[0]
    want_y, want_b = _cpu_round(x, g, buf, active, first, momentum)
    xf, yf, gf, bf = _device_round(dev, x, g, buf, active, first, momentum, ld, fused=True)
    _, ys, _, bs = _device_round(dev, x, g, buf, active, first, momentum, ld, fused=False)
    assert _same_bits(yf[:, :p], want_y), "fused != CPU restatement"
    assert _same_bits(yf[:, :p], ys[:, :p]), "fused != the three ops in sequence"
    assert _same_bits(bf[:, :p], want_b) and _same_bits(bf[:, :p], bs[:, :p])
    # untouched: x and g, the pad columns of y and buf, buf rows of inactive nodes
    assert torch.equal(xf[:, :p].view(torch.int32), x.view(torch.int32))
    assert torch.equal(gf[:, :p].view(torch.int32), g.view(torch.int32))
    for full in (xf, yf, gf, bf):
        assert bool((full[:, p:] == SENT).all())
    idle = [i for i in range(n) if i not in active]
    assert torch.equal(bf[idle, :p].view(torch.int32), buf[idle].view(torch.int32))
    if not momentum:
        assert torch.equal(bf[:, :p].view(torch.int32), buf.view(torch.int32))
    return yf[:, :p]


SHAPES = [(5, 1, 1, 1), (7, 3, 5, 7), (9, 9, 1023, 1023), (33, 8, 1028, 1032), (130, 64, 4100, 4100)]


@pytest.mark.parametrize("momentum", [0.0, MOM])
@pytest.mark.parametrize("n,k,p,ld", SHAPES)
def test_matches_sequence_and_cpu(gpu, n, k, p, ld, momentum):
    gen = torch.Generator().manual_seed(100 * n + k)
    x, g, buf = (torch.randn(n, p, generator=gen) for _ in range(3))
    active = torch.randperm(n, generator=gen)[:k].tolist()          # a shuffled order
    first = [(j % 3 == 0) for j in range(k)]                        # mixed flags
    assert active != sorted(active) or k == 1
    _check(gpu, x, g, buf, active, first, momentum, ld)


def test_order_of_the_sample_is_the_summation_order(gpu):
    gen = torch.Generator().manual_seed(7)
    n, k, p = 12, 7, 512
    x, g, buf = (torch.randn(n, p, generator=gen) * 10.0 ** torch.randint(-3, 4, (n, p), generator=gen).float()
                 for _ in range(3))
    active = torch.randperm(n, generator=gen)[:k].tolist()
    first = [False] * k
    fwd, _ = _cpu_round(x, g, buf, active, first, MOM)
    rev, _ = _cpu_round(x, g, buf, active[::-1], first, MOM)
    assert not torch.equal(fwd.view(torch.int32), rev.view(torch.int32))      # the orders do differ
    assert _same_bits(_check(gpu, x, g, buf, active, first, MOM, p), fwd)
    assert _same_bits(_check(gpu, x, g, buf, active[::-1], first, MOM, p), rev)


@pytest.mark.parametrize("momentum", [0.0, MOM])
def test_zero_signs_and_non_finite_values(gpu, momentum):
    """-0.0 in p and g of active and inactive rows (one column averages to exactly -0), inf / NaN
    in an inactive row's x (that row alone becomes NaN), inf in an active row (first of the
    sample: the whole column is NaN; later in it: the CPU arithmetic decides)."""
    gen = torch.Generator().manual_seed(3)
    n, p = 8, 12
    active, first = [5, 1, 6], [True, False, True]
    x, g = torch.randn(n, p, generator=gen), torch.randn(n, p, generator=gen)
    buf = torch.randn(n, p, generator=gen)
    x[:, 0], g[:, 0], buf[:, 0] = -0.0, 0.0, 0.0       # every t_j = -0: the average is exactly -0
    x[2, 0] = 0.0                                      # an inactive +0 row: (+0) + (-0) = +0
    x[:, 1], g[:, 1], buf[:, 1] = -0.0, -0.0, -0.0     # t_j = +0
    x[:, 2], g[:, 2], buf[:, 2] = 0.0, 0.0, -0.0
    x[[1, 3], 2] = -0.0
    g[[5, 4], 2] = -0.0
    x[3, 3] = float("inf")                             # inactive rows
    x[4, 4] = float("nan")
    x[0, 5] = float("-inf")
    x[5, 6] = float("inf")                             # active[0]
    x[6, 7] = float("inf")                             # active[2]
    g[1, 8] = float("inf")                             # an active row's gradient
    x[:, 9], g[:, 9] = 1.0, 0.0                        # cancels to an exact zero average:
    x[1, 9], x[6, 9] = -1.0, 0.0                       # 1/3 - 1/3 + 0
    buf[:, 9] = 0.0
    y = _check(gpu, x, g, buf, active, first, momentum, 12)
    assert y[:, 0].view(torch.int32).tolist() == [-2 ** 31 if i != 2 else 0 for i in range(n)]
    for col, row in ((3, 3), (4, 4), (5, 0)):
        nan = torch.isnan(y[:, col])
        assert bool(nan[row]) and int(nan.sum()) == 1, col
    assert bool(torch.isnan(y[:, 6]).all())
    assert bool(torch.isnan(y[6, 7])) and bool(torch.isinf(y[[0, 1, 2, 3, 4, 5, 7], 7]).all())
    assert bool((y[:, 10:] == y[0, 10:]).all()) and bool(torch.isfinite(y[:, 10:]).all())


def test_op_refuses_bad_arguments(gpu):
    from niidmix import ops
    z = lambda *s: torch.zeros(*s, device=gpu)  # noqa: E731
    x, y, g, b = z(4, 8), z(4, 8), z(4, 8), z(4, 8)
    act = torch.tensor([2, 0], dtype=torch.int32, device=gpu)
    fl = torch.zeros(2, dtype=torch.int32, device=gpu)
    ops.sample_step_mean_update(x, y, g, None, act, None, -LR, 0.0)
    ops.sample_step_mean_update(x, y, g, b, act, fl, -LR, MOM)
    for bad in (lambda: ops.sample_step_mean_update(x, x, g, b, act, fl, -LR, MOM),
                lambda: ops.sample_step_mean_update(x, y, g, None, act, None, -LR, MOM),
                lambda: ops.sample_step_mean_update(x, y, y, b, act, fl, -LR, MOM),
                lambda: ops.sample_step_mean_update(x, y, g, g, act, fl, -LR, MOM),
                lambda: ops.sample_step_mean_update(x, y, g, b, act[:0], fl[:0], -LR, MOM),
                lambda: ops.sample_step_mean_update(x, y, g, b, act, fl[:1], -LR, MOM),
                lambda: ops.sample_step_mean_update(x, y, g, b, act.long(), fl, -LR, MOM),
                lambda: ops.sample_step_mean_update(x.cpu(), y, g, b, act, fl, -LR, MOM),
                lambda: ops.sample_step_mean_update(x, z(4, 7), g, b, act, fl, -LR, MOM)):
        with pytest.raises(RuntimeError):
            bad()
    torch.cuda.synchronize()
