"""niidmix::gnlenet_nll_grad_rows_mfma on the GPU: tests/test_gpu_train_gnlenet.py's yardstick and
cases, the plain op's bits elsewhere, contracts, bands, one round under the new flag."""
import math

import pytest
import torch

import test_gpu_train_gnlenet as tg
from test_gpu_train_gnlenet import CASES, _bits, _check_accuracy, add_references, make_case

pytestmark = pytest.mark.gpu

PLAIN, MFMA = "gnlenet_nll_grad_rows", "gnlenet_nll_grad_rows_mfma"
_ids = ["x".join(map(str, c[:4])) for c in CASES]


def _launch(op, d, dev, **kw):
    """tg._launch (its slab, sentinels and return values) with the op `op` in the plain op's place."""
    from niidmix import ops  # noqa: F401  (registers the ops)
    with pytest.MonkeyPatch.context() as m:
        m.setattr(torch.ops.niidmix, PLAIN, getattr(torch.ops.niidmix, op))
        return tg._launch(d, dev, **kw)


@pytest.mark.parametrize("i", range(len(CASES)), ids=_ids)
def test_kernel_against_float64(i, gpu):
    d = tg._case(i)
    grad, loss, perm, before, after = _launch(MFMA, d, gpu)
    tg._check_sentinels(d, grad, perm, before, after)
    _check_accuracy(d, grad, loss, perm, f"mfma {_ids[i]}")


@pytest.mark.parametrize("i", [0, 2, 3], ids=[_ids[0], _ids[2], _ids[3]])
def test_only_the_two_weight_gradients_move(i, gpu):
    d = tg._case(i)
    new, old = _launch(MFMA, d, gpu), _launch(PLAIN, d, gpu)
    off, p = d["off"], d["p"]
    same = torch.ones(new[0].shape[1], dtype=torch.bool)            # pad columns and sentinels too
    same[off[4]:off[5]] = same[off[8]:off[9]] = False               # conv2.weight, conv3.weight
    assert torch.equal(_bits(new[0][:, same]), _bits(old[0][:, same]))
    assert torch.equal(_bits(new[1]), _bits(old[1]))
    assert not torch.equal(new[0][:, :p], old[0][:, :p])             # another summation order


def test_contracts(gpu):
    """Repeat, row alone, list in two calls: the same bits; length 0: zero gradient, NaN loss; an
    inf in one row's conv2.weight stays in that row."""
    d = tg._case(0)
    p, n = d["p"], d["n_rows"]
    a, b = _launch(MFMA, d, gpu), _launch(MFMA, d, gpu)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    perm = a[2]
    for order in ([0], [1], [2], [2, 0], [1]):                      # alone; the list cut as [2, 0] + [1]
        g, ls = _launch(MFMA, d, gpu, order=order)[:2]
        for k, r in enumerate(order):
            assert torch.equal(_bits(g[perm[r], :p]), _bits(a[0][perm[r], :p])), (order, r)
            assert torch.equal(_bits(ls[k]), _bits(a[1][r])), (order, r)
    g, ls = _launch(MFMA, d, gpu, lens=[d["lens"][0], 0, d["lens"][2]])[:2]
    assert bool((g[perm[1], :p] == 0).all()) and math.isnan(float(ls[1]))
    assert torch.equal(_bits(g[perm[0], :p]), _bits(a[0][perm[0], :p]))
    theta = d["theta"].clone()
    theta[1, d["off"][4] + 321] = float("inf")
    g, ls = _launch(MFMA, d, gpu, theta=theta)[:2]
    assert not bool(torch.isfinite(g[perm[1], :p]).all())
    for r in (0, 2):
        assert torch.equal(_bits(g[perm[r], :p]), _bits(a[0][perm[r], :p])), r
        assert torch.equal(_bits(ls[r]), _bits(a[1][r])), r


# conv2 in bands of 7, 7, 7, 7, 3 rows (31 x 31 maps) and of 7, 7, 5 (19 x 26); batches of 5 and 1
@pytest.mark.parametrize("case", [(4, 64, 64, 3, 1, 3, (3,), 611), (1, 39, 53, 3, 1, 2, (2,), 612),
                                  (1, 15, 15, 3, 2, 5, (5, 1), 613)],
                         ids=["4x64x64", "1x39x53", "1x15x15-b5-b1"])
def test_bands_and_tile_boundaries(case, gpu):
    d = add_references(make_case(*case))
    grad, loss, perm, before, after = _launch(MFMA, d, gpu)
    tg._check_sentinels(d, grad, perm, before, after)
    _check_accuracy(d, grad, loss, perm, "mfma " + "x".join(map(str, case[:3])))


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_one_round_equals_its_parts(momentum, gpu, oracle_mod, monkeypatch):
    """The flag on, the family's rule sending every shape to the new op: the models equal
    mix(step(theta, g)) with g from a direct call of the new op, bit for bit."""
    from niidmix import d_sgd, family, train
    monkeypatch.setattr(family.GN_LENET, "GRAD_MFMA_FASTER", {"map": True, "bands": True})
    monkeypatch.setattr(torch.ops.niidmix, PLAIN, getattr(torch.ops.niidmix, MFMA))   # tg._parts_round's op

    init = d_sgd.init                  # tg._setup's params get the new key before init reads them
    monkeypatch.setattr(d_sgd, "init", lambda n, t, p: (
        p["algorithm"].update({"device-training-gn-lenet-mfma": True}), init(n, t, p))[1])
    params, nodes, topo, state = tg._setup("gn", momentum)
    state, losses, _, _ = d_sgd.next_step(state, params, None)
    d_sgd.synchronize()
    got = tg._flat(nodes)
    params2, twin, topo2, _ = tg._setup("gn", momentum)
    batches, _ = train.draw(twin, params2)
    want, loss = tg._parts_round(tg._flat(twin), batches, topo2, twin, momentum, gpu, oracle_mod)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert [losses[r] for r in range(tg.N)] == loss.tolist()
