"""niidmix::gnlenet_nll_grad_rows_mfma_conv1 on the GPU under tests/test_gpu_train_gnlenet.py's yardstick."""
import math

import pytest
import torch

import test_gpu_train_gnlenet as tg
from test_gpu_train_gnlenet_mfma_sample import LIMIT

pytestmark = pytest.mark.gpu

PLAIN, BASE, NEW = "gnlenet_nll_grad_rows", "gnlenet_nll_grad_rows_mfma_sample", "gnlenet_nll_grad_rows_mfma_conv1"
_ids = ["x".join(map(str, c[:4])) for c in tg.CASES]


def _launch(d, dev, op=NEW, **kw):
    from niidmix import ops  # noqa: F401  (registers the ops)
    with pytest.MonkeyPatch.context() as m:
        m.setattr(torch.ops.niidmix, PLAIN, getattr(torch.ops.niidmix, op))
        return tg._launch(d, dev, **kw)


@pytest.mark.parametrize("what", _ids + ["pool-ties", "4x42x41"])
def test_kernel_against_float64(what, gpu):
    """Cin 1..4: 1..4 N-tiles with 25, 18, 11, 4 live lanes in the last; one band and several."""
    if what in _ids:
        d = tg._case(_ids.index(what))
    elif what == "pool-ties":          # the first pool's windows tie: the gather reads the first maximum
        d = tg.add_references(tg.make_case(1, 28, 28, 10, 2, 3, (3, 2), 2100, background=True))
    else:
        d = tg.make_case(*LIMIT)
        e_act, gap, mag = tg.separation(d["theta"][0], d["x"][d["idx"][0, :3]])
        assert gap > 16 * e_act and mag > 16 * e_act, \
            f"reseed the case: e_act {e_act:.3g}, pool gap {gap:.3g}, pre-ReLU magnitude {mag:.3g}"
        d = tg.add_references(d)
    grad, loss, perm, before, after = _launch(d, gpu)
    tg._check_sentinels(d, grad, perm, before, after)
    tg._check_accuracy(d, grad, loss, perm, "mfma-conv1 " + what)


@pytest.mark.parametrize("what", ["1x28x28x10", "3x32x32x10"])
def test_only_conv1_weight_moves(what, gpu):
    d = tg._case(_ids.index(what))
    (g, ls, perm), (g0, ls0, _) = _launch(d, gpu)[:3], _launch(d, gpu, op=BASE)[:3]
    lo, hi = d["off"][0], d["off"][1]
    assert torch.equal(tg._bits(ls), tg._bits(ls0))
    for part in (slice(0, lo), slice(hi, None)):
        assert torch.equal(tg._bits(g[:, part]), tg._bits(g0[:, part]))
    for r in range(d["n_rows"]):
        assert bool((g[perm[r], lo:hi] != 0).any())


def test_contracts(gpu):
    """Repeat, row alone, list in two calls: equal bits; a batch of length 0 between two others."""
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
    g, ls = _launch(d, gpu, lens=[d["lens"][0], 0, d["lens"][2]])[:2]
    assert bool((g[perm[1], :p] == 0).all()) and math.isnan(float(ls[1]))
    for r in (0, 2):
        assert torch.equal(bits(g[perm[r], :p]), bits(a[0][perm[r], :p])) and torch.equal(bits(ls[r]), bits(a[1][r]))


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_one_round_equals_its_parts(momentum, gpu, oracle_mod, monkeypatch):
    """The four flags on, every class routed: mix(step(theta, g)), g from the new op, bit for bit."""
    from niidmix import d_sgd, family, ops, train
    monkeypatch.setattr(family, "GRAD_MFMA_SAMPLE_FASTER", {4: True, 2: True})
    monkeypatch.setattr(family, "GRAD_MFMA_CONV1_FASTER", {4: True, 2: True})
    monkeypatch.setattr(torch.ops.niidmix, PLAIN, getattr(torch.ops.niidmix, NEW))    # tg._parts_round's op
    init = d_sgd.init                  # tg._setup's params get the new keys before init reads them
    monkeypatch.setattr(d_sgd, "init", lambda n, t, p: (
        p["algorithm"].update({"device-training-gn-lenet-mfma": True,
                               "device-training-gn-lenet-mfma-sample": True,
                               "device-training-gn-lenet-mfma-conv1": True}), init(n, t, p))[1])
    params, nodes, topo, state = tg._setup("gn", momentum)
    state, losses, _, _ = d_sgd.next_step(state, params, None)
    d_sgd.synchronize()
    assert d_sgd._trainers[id(nodes)].plan.op is ops.gnlenet_nll_grad_rows_mfma_conv1
    got = tg._flat(nodes)
    params2, twin, topo2, _ = tg._setup("gn", momentum)
    batches, _ = train.draw(twin, params2)
    want, loss = tg._parts_round(tg._flat(twin), batches, topo2, twin, momentum, gpu, oracle_mod)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert [losses[r] for r in range(tg.N)] == loss.tolist()
