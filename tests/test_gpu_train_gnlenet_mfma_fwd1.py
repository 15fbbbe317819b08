"""niidmix::gnlenet_nll_grad_rows_mfma_fwd1 on the GPU under tests/test_gpu_train_gnlenet.py's yardstick."""
import functools

import pytest
import torch

import test_gpu_train_gnlenet as tg
import test_gpu_train_gnlenet_mfma_conv1 as tc
from test_gpu_train_gnlenet_mfma_sample import LIMIT

pytestmark = pytest.mark.gpu

PLAIN, NEW = "gnlenet_nll_grad_rows", "gnlenet_nll_grad_rows_mfma_fwd1"
_ids = ["x".join(map(str, c[:4])) for c in tg.CASES]
# Cin 2 (even K), even H and W in different residues mod 4: the last row and column lie in no window,
# M-tiles straddle the rows of 15 columns, the pitch 18 is no multiple of 4.  Seeded for tg.separation
EVEN = (2, 18, 16, 5, 2, 3, (3, 2), 4100)
_launch = functools.partial(tc._launch, op=NEW)


def _separated(case):
    d = tg.make_case(*case)
    for r in range(d["n_rows"]):
        e_act, gap, mag = tg.separation(d["theta"][r], d["x"][d["idx"][r, :d["lens"][r]]])
        assert gap > 16 * e_act and mag > 16 * e_act, \
            f"reseed the case: e_act {e_act:.3g}, pool gap {gap:.3g}, pre-ReLU magnitude {mag:.3g}"
    return tg.add_references(d)


@pytest.mark.parametrize("what", _ids + ["pool-ties", "4x42x41", "2x18x16"])
def test_kernel_against_float64(what, gpu):
    if what in _ids:
        d = tg._case(_ids.index(what))
    elif what == "pool-ties":          # conv1 is exactly its bias on the background: the first maximum decides
        d = tg.add_references(tg.make_case(1, 28, 28, 10, 2, 3, (3, 2), 2100, background=True))
    else:
        d = _separated(LIMIT if what == "4x42x41" else EVEN)
    grad, loss, perm, before, after = _launch(d, gpu)
    tg._check_sentinels(d, grad, perm, before, after)
    tg._check_accuracy(d, grad, loss, perm, "mfma-fwd1 " + what)


def test_contracts(gpu):
    """Repeat, row alone, list in two calls: equal bits; length 0; an inf in row 1's conv1.weight."""
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
    theta[1, d["off"][0] + 7] = float("inf")
    for kw in (dict(lens=[d["lens"][0], 0, d["lens"][2]]), dict(theta=theta)):
        g, ls = _launch(d, gpu, **kw)[:2]
        assert (bool((g[perm[1], :p] == 0).all()) and bool(ls[1] != ls[1])) if "lens" in kw else \
            not bool(torch.isfinite(g[perm[1], :p]).all())
        for r in (0, 2):
            assert torch.equal(bits(g[perm[r], :p]), bits(a[0][perm[r], :p])), (list(kw), r)
            assert torch.equal(bits(ls[r]), bits(a[1][r])), (list(kw), r)


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_one_round_equals_its_parts(momentum, gpu, oracle_mod, monkeypatch):
    from niidmix import d_sgd, family, ops, train
    for table in ("GRAD_MFMA_SAMPLE_FASTER", "GRAD_MFMA_CONV1_FASTER", "GRAD_MFMA_FWD1_FASTER"):
        monkeypatch.setattr(family, table, {4: True, 2: True})
    monkeypatch.setattr(torch.ops.niidmix, PLAIN, getattr(torch.ops.niidmix, NEW))    # tg._parts_round's op
    init = d_sgd.init                  # tg._setup's params get the new keys before init reads them
    monkeypatch.setattr(d_sgd, "init", lambda n, t, p: (
        p["algorithm"].update({"device-training-gn-lenet-mfma" + k: True
                               for k in ("", "-sample", "-conv1", "-fwd1")}), init(n, t, p))[1])
    params, nodes, topo, state = tg._setup("gn", momentum)
    state, losses, _, _ = d_sgd.next_step(state, params, None)
    d_sgd.synchronize()
    assert d_sgd._trainers[id(nodes)].plan.op is ops.gnlenet_nll_grad_rows_mfma_fwd1
    got = tg._flat(nodes)
    params2, twin, topo2, _ = tg._setup("gn", momentum)
    batches, _ = train.draw(twin, params2)
    want, loss = tg._parts_round(tg._flat(twin), batches, topo2, twin, momentum, gpu, oracle_mod)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert [losses[r] for r in range(tg.N)] == loss.tolist()
