"""--learning-momentum on the device, the host side (no GPU): which optimizers the device step
accepts, and the arithmetic contract k_sgd_momentum_step_rows implements."""
import numpy as np
import torch


def _nodes(params, n=3, **kw):
    from niidmix import d_sgd
    out = []
    for r in range(n):
        m = torch.nn.Linear(4, 2)
        opt = d_sgd.optimizer(m, params) if not kw else torch.optim.SGD(m.parameters(), **kw)
        out.append({"rank": r, "model": m, "optimizer": opt})
    return out


def _cpu_step(node):
    node["optimizer"].zero_grad()
    node["model"](torch.ones(1, 4)).sum().backward()
    node["optimizer"].step()


def test_device_step_eligibility_with_momentum(monkeypatch):
    """_device_step_ok takes a non-zero momentum exactly when the optimizer's equals params'
    learning-momentum (the rule for the learning rate); dampening, weight decay and Nesterov stay
    refused, and so is a node list of which only some optimizers hold momentum state."""
    from niidmix import d_sgd
    monkeypatch.delenv("NIIDMIX_DEVICE_STEP", raising=False)
    monkeypatch.delenv("NIIDMIX_RESIDENT", raising=False)
    p9 = {"algorithm": {"learning-rate": 0.1, "learning-momentum": 0.9}}
    p0 = {"algorithm": {"learning-rate": 0.1, "learning-momentum": 0.0}}
    assert d_sgd._device_step_ok(p9, _nodes(p9))
    assert d_sgd._device_step_ok(p9, _nodes(p9, lr=0.1, momentum=0.9))
    assert not d_sgd._device_step_ok(p9, _nodes(p9, lr=0.1, momentum=0.0))
    assert not d_sgd._device_step_ok(p0, _nodes(p0, lr=0.1, momentum=0.9))
    assert not d_sgd._device_step_ok(p9, _nodes(p9, lr=0.1, momentum=0.5))
    assert not d_sgd._device_step_ok(p9, _nodes(p9, lr=0.1, momentum=0.9, nesterov=True))
    assert not d_sgd._device_step_ok(p9, _nodes(p9, lr=0.1, momentum=0.9, dampening=0.1))
    assert not d_sgd._device_step_ok(p9, _nodes(p9, lr=0.1, momentum=0.9, weight_decay=1e-4))
    assert not d_sgd._device_step_ok(p9, _nodes(p9, lr=0.2, momentum=0.9))
    # momentum state: all or none is fine, some is not
    nd = _nodes(p9)
    _cpu_step(nd[1])
    assert d_sgd._momentum_state(nd) == "mixed"
    assert not d_sgd._device_step_ok(p9, nd)
    _cpu_step(nd[0])
    _cpu_step(nd[2])
    assert d_sgd._momentum_state(nd) == "all"
    assert d_sgd._device_step_ok(p9, nd)
    nd = _nodes(p9)
    first = next(iter(nd[0]["model"].parameters()))
    nd[0]["optimizer"].state[first]["momentum_buffer"] = torch.zeros_like(first)
    assert not d_sgd._device_step_ok(p9, nd)          # one parameter of one node only
    monkeypatch.setenv("NIIDMIX_DEVICE_STEP", "0")
    assert not d_sgd._device_step_ok(p9, _nodes(p9))


def test_fused_eligibility_with_momentum(monkeypatch):
    """_fused_ok: gradient averaging with momentum takes the fused round (resident engine only),
    for the plugin's optimizer at params' momentum."""
    from niidmix import d_sgd
    monkeypatch.delenv("NIIDMIX_FUSED", raising=False)
    monkeypatch.delenv("NIIDMIX_RESIDENT", raising=False)
    for flag in ("clique-gradient", "unbiased-gradient"):
        p9 = {"algorithm": {"learning-rate": 0.1, "learning-momentum": 0.9, flag: True}}
        assert d_sgd._fused_ok(p9)
        assert d_sgd._fused_ok(p9, _nodes(p9))
        assert not d_sgd._fused_ok(p9, _nodes(p9, lr=0.1, momentum=0.0))
        assert not d_sgd._fused_ok(p9, _nodes(p9, lr=0.1, momentum=0.9, nesterov=True))
    p9 = {"algorithm": {"learning-rate": 0.1, "learning-momentum": 0.9, "clique-gradient": True}}
    assert not d_sgd._fused_ok({"algorithm": {"learning-rate": 0.1, "learning-momentum": 0.9}})
    monkeypatch.setenv("NIIDMIX_RESIDENT", "0")       # the windowed runner has no momentum
    assert not d_sgd._fused_ok(p9)
    monkeypatch.delenv("NIIDMIX_RESIDENT")
    monkeypatch.setenv("NIIDMIX_FUSED", "0")
    assert not d_sgd._fused_ok(p9)


def test_engine_key_has_momentum():
    from niidmix import d_sgd
    a = {"algorithm": {"learning-rate": 0.1, "learning-momentum": 0.9}}
    b = {"algorithm": {"learning-rate": 0.1, "learning-momentum": 0.5}}
    assert d_sgd._fused_key(a, True) != d_sgd._fused_key(b, True)
    assert d_sgd._fused_key(a, True) == d_sgd._fused_key(dict(a), True)


def _fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, for finite fp32 arrays: the product is exact in float64;
    the float64 sum is corrected to round-to-odd from its exact error (TwoSum), after which the
    rounding to fp32 equals the rounding of the exact value (53 >= 2 * 24 + 2 bits)."""
    s = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    t = s + c
    bb = t - s
    err = (s - (t - bb)) + (c - bb)
    ti = t.view(np.int64)
    toward_zero = np.where((err == 0) | ((err > 0) == (t > 0)), ti, ti - 1)
    odd = np.where(err != 0, toward_zero | 1, ti)
    return odd.view(np.float64).astype(np.float32)


def test_momentum_arithmetic_contract():
    """torch.optim.SGD(momentum=m) on CPU tensors is, bit for bit,
        first step:   buf = g                              (a copy: -0.0 stays -0.0)
        later steps:  buf = fl(fl(m32 * buf) + g)          (two roundings)
        every step:   p   = fma(nlr32, buf, p)             (one rounding)
    with m32 = fp32(m), nlr32 = fp32(-lr): what include/niidmix.h promises for
    niidmix_sgd_momentum_step_rows_f32.  A later torch whose CPU kernel rounds differently fails
    here, before any GPU test does."""
    n = 20003
    for m_, lr in ((0.9, 0.07), (0.95, 0.002), (0.5, 0.1)):
        gen = torch.Generator().manual_seed(7)
        q = torch.nn.Parameter(torch.randn(n, generator=gen))
        opt = torch.optim.SGD([q], lr=lr, momentum=m_)
        p = q.detach().numpy().copy()
        buf = None
        m32, nlr32 = np.float32(m_), np.float32(-lr)
        for step in range(4):
            g = torch.randn(n, generator=gen)
            if step == 0:
                g[:5] = torch.tensor([-0.0, 0.0, -0.0, 1.0, -1.0])
            q.grad = g.clone()
            opt.step()
            gn = g.numpy()
            if buf is None:
                buf = gn.copy()
            else:
                buf = (m32 * buf).astype(np.float32) + gn          # fp32 * fp32, fp32 + fp32
            p = _fma32(np.full(n, nlr32), buf, p)
            tb = opt.state[q]["momentum_buffer"].numpy()
            assert np.array_equal(tb.view(np.int32), buf.view(np.int32)), (m_, lr, step)
            assert np.array_equal(q.detach().numpy().view(np.int32), p.view(np.int32)), (m_, lr, step)
    # the first step copies: a -0.0 gradient gives a -0.0 buffer (a zeroed buffer would give +0.0)
    q = torch.nn.Parameter(torch.ones(3))
    q.grad = torch.tensor([-0.0, 0.0, 2.0])
    opt = torch.optim.SGD([q], lr=0.1, momentum=0.9)
    opt.step()
    assert torch.signbit(opt.state[q]["momentum_buffer"]).tolist() == [True, False, False]
