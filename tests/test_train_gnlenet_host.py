"""--device-training-gn-lenet, the parts that need no GPU: the flag, its acceptance and refusals,
the float64 yardstick (niidmix.train.fp64_reference_gn_lenet) pinned to the reference's own
gradients (tests/golden/gn_lenet/*_grad.npz, made by tests/golden/make_golden_gn_lenet_grad.py),
the C entry point's argument checks and scratch size, and the row-list chunking arithmetic."""
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_eval_gnlenet_host as th
from conftest import REPO

GN = "device-training-gn-lenet"


def _params(**alg):
    a = {"device-evaluation": False, "device-training": True, GN: True, "batch-size": 4}
    a.update(alg)
    return th._params(**a)


def _nodes(params, models, shape=(1, 28, 28)):
    nodes = th._nodes(params, models)
    for nd in nodes:
        nd["train-set"] = [(torch.zeros(*shape), 0)] * 4
    return nodes


def test_cli_flag_writes_both_keys(tmp_path, monkeypatch):
    from niidmix import d_sgd
    seen = {}
    monkeypatch.setattr(d_sgd.m, "rundir", lambda args: str(tmp_path))
    monkeypatch.setattr(d_sgd.m, "params", lambda rundir: {"topology": {"name": "ring"}})
    monkeypatch.setattr(d_sgd.m, "extend", lambda rundir, key, val: seen.update({key: val}))
    monkeypatch.setattr(d_sgd, "load_topology", lambda rundir: {})
    d_sgd.main(["--rundir", str(tmp_path), "--device-training-gn-lenet"])
    assert seen["algorithm"][GN] is True and seen["algorithm"]["device-training"] is True
    d_sgd.main(["--rundir", str(tmp_path)])
    assert GN not in seen["algorithm"] and "device-training" not in seen["algorithm"]
    d_sgd.main(["--rundir", str(tmp_path), "--device-training"])
    assert GN not in seen["algorithm"] and seen["algorithm"]["device-training"] is True
    json.dumps(seen["algorithm"])


def test_check_eligible_accepts_gn_lenet_under_the_new_key():
    from niidmix import d_sgd, train
    p = _params()
    nodes = _nodes(p, [th.GNLeNet(), th.GNLeNet()])
    assert train.check_eligible(nodes, p) == (1, 10, 256)
    state, _, _ = d_sgd.init(nodes, {"edges": {}}, p)
    idx = next(nodes[0]["train-iterator"])
    assert idx.dtype == torch.int64 and idx.dim() == 1               # index loaders, as for linear
    p3 = _params()
    assert train.check_eligible(_nodes(p3, [th.GNLeNet(3, 10, (32, 32))] * 2, (3, 32, 32)), p3) == (3, 10, 576)
    # an all-linear list under the new key: (K, C) as before
    assert train.check_eligible(_nodes(p, [th.Net(), th.Net()]), p) == (784, 10)


def test_the_plain_flag_names_the_new_one():
    from niidmix import train
    p = _params(**{GN: False})
    with pytest.raises(ValueError, match=r"--device-training .*--device-training-gn-lenet"):
        train.check_eligible(_nodes(p, [th.GNLeNet(), th.GNLeNet()]), p)


def test_refusals_under_the_new_key(monkeypatch):
    from niidmix import d_sgd, train
    two = lambda: [th.GNLeNet(), th.GNLeNet()]  # noqa: E731

    def refused(p, nodes, match=GN):
        with pytest.raises(ValueError, match=match):
            train.check_eligible(nodes, p)

    p = _params()
    p["topology"]["name"] = "sample"
    refused(p, _nodes(p, two()))
    for key in ("clique-gradient", "unbiased-gradient"):
        p = _params(**{key: True})
        refused(p, _nodes(p, two()))
    p = _params()
    monkeypatch.setenv("NIIDMIX_DEVICES", "0,1")
    refused(p, _nodes(p, two()))
    monkeypatch.delenv("NIIDMIX_DEVICES")
    refused(p, [])
    nodes = _nodes(p, two())
    nodes[1]["optimizer"] = torch.optim.Adam(nodes[1]["model"].parameters(), lr=0.1)     # foreign
    refused(p, nodes)
    for models in ([th.GNLeNet(), th.Net()], [th.Net(), th.GNLeNet()], [th.GNLeNet(), th.GNLeNet(c=9)],
                   [th.GNLeNet(), th.GNLeNet(hw=(32, 32))], [th.GNLeNet(), th.GNLeNet(cin=3)],
                   [th.GNLeNet(c=1025)], [th.GNLeNet(cin=5)]):
        shape = (models[0].features[0].in_channels, 28, 28) if isinstance(models[0], th.GNLeNet) else (1, 28, 28)
        refused(p, _nodes(p, models, shape))
    # samples that are not [Cin, H, W] with H, W in [15, 64], or do not give the classifier's F
    for shape in ((784,), (28, 28), (2, 28, 28), (1, 14, 28), (1, 28, 65)):
        refused(p, _nodes(p, two(), shape))
    refused(p, _nodes(p, two(), (1, 32, 32)), match=GN + ".*F = 256")
    assert train.check_eligible(_nodes(p, two(), (1, 24, 24)), p) == (1, 10, 256)         # F fits
    # live CPU momentum buffers: DeviceTrainer's refusal, stated without a GPU by its predicate
    pm = _params(**{"learning-momentum": 0.9})
    nodes = _nodes(pm, two())
    F.nll_loss(nodes[0]["model"].forward(torch.zeros(2, 1, 28, 28), pm), torch.zeros(2, dtype=torch.int64)).backward()
    nodes[0]["optimizer"].step()
    assert d_sgd._momentum_state(nodes) != "none"


@pytest.mark.parametrize("name", ["gn_lenet_mnist", "gn_lenet_cifar"])
def test_float64_gradient_reproduces_the_reference(name):
    """Per tensor max|g64 - g_ref| <= 1e-3 max|g_ref| and the loss within 1e-5; the measured values
    are near 1e-6 (the reference's fp32 rounding)."""
    from niidmix import train
    f, g = th.load_fixture(name), th.load_fixture(name + "_grad")
    cin, h, w, c = (int(v) for v in f["shape"])
    theta, x, y = torch.from_numpy(f["theta"]), torch.from_numpy(f["x"]), torch.from_numpy(f["y"])
    assert g["grad"].dtype == np.float32 and g["grad"].shape == f["theta"].shape
    l64, g64 = train.fp64_reference_gn_lenet(theta, x, y)
    assert g64.dtype == torch.float64 and g64.shape == theta.shape
    ref = torch.from_numpy(g["grad"]).double()
    off = train.gn_lenet_offsets(cin, c, th.sizes(cin, h, w, c)[0])
    worst = 0.0
    for t in range(14):
        s = slice(off[t], off[t + 1])
        r = float((g64[s] - ref[s]).abs().max()) / float(ref[s].abs().max())
        worst = max(worst, r)
        assert r <= 1e-3, (t, r)
    dl = abs(float(l64) - float(g["loss"]))
    print(f"{name}: worst per-tensor |g64 - g_ref| / max|g_ref| = {worst:.3g}, |loss64 - loss_ref| = {dl:.3g}")
    assert dl <= 1e-5


@pytest.mark.parametrize("cin,c,hw", [(1, 3, (15, 15)), (3, 10, (17, 15)), (1, 10, (28, 28))])
def test_float64_gradient_against_the_local_module(cin, c, hw):
    """The same yardstick against autograd of the locally built module (registration order, layer
    order): fp32 module against float64 restatement, 1e-3 per tensor as above."""
    from niidmix import train
    gen = torch.Generator().manual_seed(11)
    torch.manual_seed(12)
    mdl = th.perturb(th.GNLeNet(cin, c, hw), gen)
    x = torch.randn(3, cin, *hw, generator=gen)
    y = torch.randint(0, c, (3,), generator=gen)
    loss = F.nll_loss(mdl.forward(x, {}), y)
    loss.backward()
    theta = torch.cat([q.detach().reshape(-1) for q in mdl.parameters()])
    l64, g64 = train.fp64_reference_gn_lenet(theta, x, y)
    assert abs(float(l64) - float(loss.detach())) <= 1e-5 * max(1.0, abs(float(l64)))
    off = train.gn_lenet_offsets(cin, c, th.sizes(cin, hw[0], hw[1], c)[0])
    for t, q in enumerate(mdl.parameters()):
        d = float((g64[off[t]:off[t + 1]] - q.grad.reshape(-1).double()).abs().max())
        assert d <= 1e-3 * float(q.grad.abs().max()), (t, d)
    with pytest.raises(ValueError):
        train.split_gn_lenet(theta[:-1], cin, hw)


def test_gnlenet_grad_argument_errors_without_gpu():
    """Validation happens before any HIP call, in the order include/niidmix.h documents; the
    made-up addresses are never dereferenced."""
    from niidmix import _lib
    L = _lib.lib
    Fn = L.niidmix_gnlenet_nll_grad_rows_f32
    B = L.niidmix_gnlenet_nll_grad_rows_scratch_bytes
    base, far, lss, scr = 1 << 20, 1 << 30, 1 << 36, 1 << 40
    n, bm, p = 2, 5, 80554

    def call(theta=base, ld_t=None, data=8, labels=8, idx=8, length=8, b_max=bm, rows=8, n_rows=n,
             grad=far, ld_g=None, loss=lss, Cin=1, H=28, W=28, C=10, scratch=scr, nbytes=None):
        wide = p if (Cin, H, W, C) == (1, 28, 28, 10) else 1 << 24
        if nbytes is None:
            nbytes = B(max(n_rows, 1), max(b_max, 1), Cin, H, W, C)
        return Fn(theta, wide if ld_t is None else ld_t, data, labels, idx, length, b_max, rows, n_rows,
                  grad, wide if ld_g is None else ld_g, loss, Cin, H, W, C, scratch, nbytes, None)

    def err():
        return L.niidmix_last_error()

    for name in ("theta", "data", "labels", "idx", "length", "rows", "grad", "loss", "scratch"):
        assert call(**{name: None}) == _lib.EINVAL and b"null" in err(), name
    for name in ("n_rows", "b_max", "Cin", "H", "W", "C"):
        for v in (0, -1):
            assert call(**{name: v}) == _lib.EINVAL and b">= 1" in err(), name
    assert call(n_rows=0, theta=None) == _lib.EINVAL and b"null" in err()          # null before sizes
    assert call(C=1025) == _lib.EUNSUPPORTED and b"C 1025" in err()
    assert call(Cin=5) == _lib.EUNSUPPORTED and b"Cin 5" in err()
    for hw in (14, 65, 1):
        assert call(H=hw) == _lib.EUNSUPPORTED and b"H" in err()
        assert call(W=hw) == _lib.EUNSUPPORTED
    assert call(b_max=1 << 31) == _lib.EUNSUPPORTED and b"b_max" in err()
    assert call(n_rows=1 << 25, nbytes=1) == _lib.EUNSUPPORTED and b"n_rows" in err()
    assert call(b_max=(1 << 24) + 1) == _lib.EUNSUPPORTED and b"b_max" in err()
    # 2^32 (row, tile) slots: refused before the size could wrap; the size function gives 0
    assert call(n_rows=1 << 12, b_max=1 << 21, nbytes=1) == _lib.EUNSUPPORTED and b"slots" in err()
    assert B(1 << 12, 1 << 21, 1, 28, 28, 10) == 0 and B(1 << 24, 1 << 24, 3, 64, 64, 1024) == 0
    big = B(1 << 20, 4094, 3, 64, 64, 1024)                     # 2^20 x 2047 slots: the largest sizes
    assert big == (1 << 20) * 2047 * (B(1, 2, 3, 64, 64, 1024)) and 0 < big < 1 << 53
    assert call(H=0, C=1025) == _lib.EINVAL                                       # sizes before limits
    assert call(C=1025, ld_t=1) == _lib.EUNSUPPORTED                              # limits before ld
    assert call(ld_t=p - 1) == _lib.EINVAL and b"leading dimension < P" in err()
    assert call(ld_g=p - 1) == _lib.EINVAL and b"leading dimension < P" in err()
    assert call(ld_g=p - 1, nbytes=1) == _lib.EINVAL and b"leading" in err()      # ld before scratch
    assert call(nbytes=1) == _lib.EINVAL and b"scratch" in err()
    assert call(nbytes=B(n, bm, 1, 28, 28, 10) - 1) == _lib.EINVAL
    assert call(scratch=scr + 4) == _lib.EINVAL and b"scratch" in err()           # 8-B alignment
    assert call(grad=base, nbytes=1) == _lib.EINVAL                               # scratch before alias
    assert call(grad=base) == _lib.EALIAS and b"overlap" in err()
    assert call(grad=base + 4 * (2 * p - 1)) == _lib.EALIAS                       # theta's second row
    assert call(loss=base + 4 * p) == _lib.EALIAS and b"loss or scratch" in err()
    assert call(scratch=base + 8) == _lib.EALIAS
    assert call(scratch=far + 8) == _lib.EALIAS and b"scratch overlaps grad" in err()


def test_gnlenet_grad_scratch_bytes():
    from niidmix import _lib
    B = _lib.lib.niidmix_gnlenet_nll_grad_rows_scratch_bytes
    assert B(0, 10, 1, 28, 28, 10) == 0 and B(5, 0, 1, 28, 28, 10) == 0 and B(-1, 10, 1, 28, 28, 10) == 0
    assert B(5, 10, 0, 28, 28, 10) == 0 and B(5, 10, 1, 14, 28, 10) == 0 and B(5, 10, 1, 28, 65, 10) == 0
    assert B(5, 10, 5, 28, 28, 10) == 0 and B(5, 10, 1, 28, 28, 1025) == 0
    assert B(1, 1, 1, 15, 15, 1) > 0
    for hw in (15, 28, 32, 35, 64):
        for n, m in [(1, 1), (7, 63), (7, 64), (1000, 20), (3, 257)]:
            b = B(n, m, 3, hw, hw, 10)
            assert b > 0 and b % 16 == 0
            assert B(n + 1, m, 3, hw, hw, 10) > b
            assert B(n, m + 1, 3, hw, hw, 10) >= b and B(n, m + 2, 3, hw, hw, 10) > b
            assert B(n, m, 3, hw, hw, 11) >= b
            assert B(2 * n, m, 3, hw, hw, 10) == 2 * b                 # proportional to the rows
    per_sample = B(1000, 20, 3, 32, 32, 10) / 20000
    assert 150e3 < per_sample < 200e3                                  # about 180 KB per sample


def test_row_list_chunking():
    """train.cut_rows: all rows when they fit, else halved until the call's scratch does; None when
    one row does not fit.  With the real size function under a small budget."""
    from niidmix import _lib, train
    B = _lib.lib.niidmix_gnlenet_nll_grad_rows_scratch_bytes
    need = lambda k: int(B(k, 20, 3, 32, 32, 10))  # noqa: E731
    assert train.cut_rows(1000, need, need(1000)) == 1000
    assert train.cut_rows(1000, need, need(1000) - 1) == 500
    assert train.cut_rows(1000, need, need(300)) == 250
    assert train.cut_rows(7, need, need(2)) == 2
    assert train.cut_rows(7, need, need(1)) == 1
    assert train.cut_rows(7, need, need(1) - 1) is None
    for n, budget_rows in [(1000, 33), (17, 5), (4, 2)]:
        k = train.cut_rows(n, need, need(budget_rows))
        calls = [(a, min(n, a + k)) for a in range(0, n, k)]
        assert 1 <= k <= budget_rows and calls[0][0] == 0 and calls[-1][1] == n
        assert all(b - a <= k for a, b in calls) and all(calls[i][1] == calls[i + 1][0] for i in range(len(calls) - 1))


def test_header_and_signatures_declare_the_entry():
    from niidmix import _lib, evaluate
    assert _lib.lib.niidmix_abi_version() == 6
    text = open(os.path.join(REPO, "include", "niidmix.h")).read()
    assert re.search(r"^int niidmix_gnlenet_nll_grad_rows_f32\(", text, re.M)
    assert re.search(r"^int64_t niidmix_gnlenet_nll_grad_rows_scratch_bytes\(", text, re.M)
    assert "niidmix_gnlenet_nll_grad_rows_f32" in _lib.SIGNATURES
    assert "niidmix_gnlenet_nll_grad_rows_scratch_bytes" in _lib.SIGNATURES
    # the shape helpers live in niidmix.family; evaluate keeps no alias of them
    assert not hasattr(evaluate, "gn_lenet_shape") and not hasattr(evaluate, "gn_lenet_offsets")
