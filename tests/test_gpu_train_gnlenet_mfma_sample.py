"""niidmix::gnlenet_nll_grad_rows_mfma_sample on the GPU under tests/test_gpu_train_gnlenet.py's yardstick."""
import math

import pytest
import torch

import test_gpu_train_gnlenet as tg

pytestmark = pytest.mark.gpu

PLAIN, NEW = "gnlenet_nll_grad_rows", "gnlenet_nll_grad_rows_mfma_sample"
_ids = ["x".join(map(str, c[:4])) for c in tg.CASES]
# pooled maps of 20 x 20, two tiles, the second of one sample; seeded on the CPU for tg.separation
LIMIT = (4, 42, 41, 3, 1, 3, (3,), 29200)


def _launch(d, dev, **kw):
    from niidmix import ops  # noqa: F401  (registers the ops)
    with pytest.MonkeyPatch.context() as m:
        m.setattr(torch.ops.niidmix, PLAIN, getattr(torch.ops.niidmix, NEW))
        return tg._launch(d, dev, **kw)


@pytest.mark.parametrize("what", _ids + ["pool-ties", "4x42x41"])
def test_kernel_against_float64(what, gpu):
    if what in _ids:
        d = tg._case(_ids.index(what))
    elif what == "pool-ties":          # the first pool's windows tie: the first maximum must win
        d = tg.add_references(tg.make_case(1, 28, 28, 10, 2, 3, (3, 2), 2100, background=True))
    else:
        d = tg.make_case(*LIMIT)
        e_act, gap, mag = tg.separation(d["theta"][0], d["x"][d["idx"][0, :3]])
        assert gap > 16 * e_act and mag > 16 * e_act, \
            f"reseed the case: e_act {e_act:.3g}, pool gap {gap:.3g}, pre-ReLU magnitude {mag:.3g}"
        d = tg.add_references(d)
    grad, loss, perm, before, after = _launch(d, gpu)
    tg._check_sentinels(d, grad, perm, before, after)
    tg._check_accuracy(d, grad, loss, perm, "mfma-sample " + what)


def test_contracts(gpu):
    """Repeat, row alone, list in two calls: equal bits; length 0; an inf in row 1's conv2.weight."""
    d = tg._case(0)
    p, bits = d["p"], tg._bits
    a, b = _launch(d, gpu), _launch(d, gpu)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))
    perm = a[2]
    for order in ([0], [1], [2], [2, 0], [1]):                      # alone; the list cut as [2, 0] + [1]
        g, ls = _launch(d, gpu, order=order)[:2]
        for k, r in enumerate(order):
            assert torch.equal(bits(g[perm[r], :p]), bits(a[0][perm[r], :p])), (order, r)
            assert torch.equal(bits(ls[k]), bits(a[1][r])), (order, r)
    theta = d["theta"].clone()
    theta[1, d["off"][4] + 321] = float("inf")
    for kw in (dict(lens=[d["lens"][0], 0, d["lens"][2]]), dict(theta=theta)):
        g, ls = _launch(d, gpu, **kw)[:2]
        assert (bool((g[perm[1], :p] == 0).all()) and math.isnan(float(ls[1]))) if "lens" in kw else \
            not bool(torch.isfinite(g[perm[1], :p]).all())
        for r in (0, 2):
            assert torch.equal(bits(g[perm[r], :p]), bits(a[0][perm[r], :p])), (list(kw), r)
            assert torch.equal(bits(ls[r]), bits(a[1][r])), (list(kw), r)


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_one_round_equals_its_parts(momentum, gpu, oracle_mod, monkeypatch):
    """The three flags on, every class routed: mix(step(theta, g)), g from the new op, bit for bit."""
    from niidmix import d_sgd, family, ops, train
    monkeypatch.setattr(family, "GRAD_MFMA_SAMPLE_FASTER", {4: True, 2: True})
    monkeypatch.setattr(torch.ops.niidmix, PLAIN, getattr(torch.ops.niidmix, NEW))    # tg._parts_round's op
    init = d_sgd.init                  # tg._setup's params get the new keys before init reads them
    monkeypatch.setattr(d_sgd, "init", lambda n, t, p: (
        p["algorithm"].update({"device-training-gn-lenet-mfma": True,
                               "device-training-gn-lenet-mfma-sample": True}), init(n, t, p))[1])
    params, nodes, topo, state = tg._setup("gn", momentum)
    state, losses, _, _ = d_sgd.next_step(state, params, None)
    d_sgd.synchronize()
    assert d_sgd._trainers[id(nodes)].plan.op is ops.gnlenet_nll_grad_rows_mfma_sample
    got = tg._flat(nodes)
    params2, twin, topo2, _ = tg._setup("gn", momentum)
    batches, _ = train.draw(twin, params2)
    want, loss = tg._parts_round(tg._flat(twin), batches, topo2, twin, momentum, gpu, oracle_mod)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert [losses[r] for r in range(tg.N)] == loss.tolist()
