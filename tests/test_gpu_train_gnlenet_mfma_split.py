"""niidmix::gnlenet_nll_grad_rows_mfma_split on the GPU under tests/test_gpu_train_gnlenet.py's yardstick.
With CH = ops.gnlenet_grad_split_chunk(shape) a long case's rows have 2 CH + 1, CH and CH + 1 samples:
three chunks with a last one of one sample, one chunk (written straight into grad), two chunks."""
import math

import pytest
import torch

import test_gpu_train_gnlenet as tg

pytestmark = pytest.mark.gpu

PLAIN, BASE, NEW = "gnlenet_nll_grad_rows", "gnlenet_nll_grad_rows_mfma_conv1", "gnlenet_nll_grad_rows_mfma_split"
# shape: seed.  Minimal pooled maps; odd, non-square, two N-tiles in conv1; the shape limit (bands,
# four N-tiles; one row of CH + 2 samples).  Seeded on the CPU so that no pool argmax and no ReLU
# sign of a case differs between float64 and torch's fp32 forward (with this many samples
# tg.separation's margin of 16 e_act cannot be asked for)
SEEDS = {(1, 15, 15, 3): 2, (3, 17, 15, 10): 1, (4, 42, 41, 3): 2}
FIRST = next(iter(SEEDS))
_cache = {}


def _long(shape):
    if shape not in _cache:
        from niidmix import ops
        ch = ops.gnlenet_grad_split_chunk(*shape)
        lens = [ch + 2] if shape[1] > 40 else [2 * ch + 1, ch, ch + 1]
        _cache[shape] = tg.add_references(tg.make_case(*shape, len(lens), max(lens), lens, SEEDS[shape]))
    return _cache[shape]


def _launch(d, dev, op=NEW, **kw):
    from niidmix import ops  # noqa: F401  (registers the ops)
    with pytest.MonkeyPatch.context() as m:
        m.setattr(torch.ops.niidmix, PLAIN, getattr(torch.ops.niidmix, op))
        return tg._launch(d, dev, **kw)


@pytest.mark.parametrize("shape,layout", [(s, "vec") for s in SEEDS] + [(FIRST, "scalar")])
def test_kernel_against_float64(shape, layout, gpu):
    d = _long(shape)
    grad, loss, perm, before, after = _launch(d, gpu, layout=layout)
    tg._check_sentinels(d, grad, perm, before, after)
    tg._check_accuracy(d, grad, loss, perm, f"mfma-split {shape} {layout}")


@pytest.mark.parametrize("i", [0, 3])
def test_short_batches_keep_the_conv1_entry_bits(i, gpu):
    d = tg._case(i)                        # batches of at most 4 samples: no chunk is cut
    (g, ls), (g0, ls0) = _launch(d, gpu)[:2], _launch(d, gpu, op=BASE)[:2]
    assert torch.equal(tg._bits(g), tg._bits(g0)) and torch.equal(tg._bits(ls), tg._bits(ls0))


def test_only_the_three_weights_move(gpu):
    d = _long(FIRST)
    (g, ls, perm), (g0, ls0, _) = _launch(d, gpu)[:3], _launch(d, gpu, op=BASE)[:3]
    off = d["off"]
    assert torch.equal(tg._bits(ls), tg._bits(ls0))
    for t in range(14):
        part = slice(off[t], off[t + 1])
        if t in (0, 4, 8):                 # conv1.weight, conv2.weight, conv3.weight
            assert all(bool((g[perm[r], part] != 0).any()) for r in range(d["n_rows"]))
        else:
            assert torch.equal(tg._bits(g[:, part]), tg._bits(g0[:, part])), t
    assert torch.equal(tg._bits(g[perm[1]]), tg._bits(g0[perm[1]]))     # one chunk: the conv1 entry's chain


def test_contracts(gpu):
    """Repeat, row alone, list in two calls: equal bits; a batch of length 0 between two long ones."""
    d = _long(FIRST)
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


def test_one_round_equals_its_parts(gpu, oracle_mod, monkeypatch):
    """The five flags on, every class routed: mix(step(theta, g)), g from the new op, bit for bit."""
    from niidmix import d_sgd, family, ops, train
    for table in ("GRAD_MFMA_SAMPLE_FASTER", "GRAD_MFMA_CONV1_FASTER", "GRAD_MFMA_SPLIT_FASTER"):
        monkeypatch.setattr(family, table, {4: True, 2: True})
    monkeypatch.setattr(torch.ops.niidmix, PLAIN, getattr(torch.ops.niidmix, NEW))    # tg._parts_round's op
    init = d_sgd.init                  # tg._setup's params get the new keys before init reads them
    monkeypatch.setattr(d_sgd, "init", lambda n, t, p: (
        p["algorithm"].update({"device-training-gn-lenet-mfma" + k: True
                               for k in ("", "-sample", "-conv1", "-split")}), init(n, t, p))[1])
    params, nodes, topo, state = tg._setup("gn", 0.9)
    state, losses, _, _ = d_sgd.next_step(state, params, None)
    d_sgd.synchronize()
    assert d_sgd._trainers[id(nodes)].plan.op is ops.gnlenet_nll_grad_rows_mfma_split
    got = tg._flat(nodes)
    params2, twin, topo2, _ = tg._setup("gn", 0.9)
    batches, _ = train.draw(twin, params2)
    want, loss = tg._parts_round(tg._flat(twin), batches, topo2, twin, 0.9, gpu, oracle_mod)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert [losses[r] for r in range(tg.N)] == loss.tolist()
