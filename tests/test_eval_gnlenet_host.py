"""--device-evaluation for GN-LeNet, the parts that need no GPU: the model's shape and row
layout, the flag's acceptance and refusals, the C entry point's argument checks and scratch size,
the header, and the float64 restatement of the forward pass that tests/test_gpu_eval_gnlenet.py
measures the kernel against, pinned here to the reference's own log-probs (tests/golden/gn_lenet,
made by tests/golden/make_golden_gn_lenet.py)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, REPO


def down(h):
    return (h - 3) // 2 + 1


def sizes(cin, h, w, c):
    """(F, P) of GN-LeNet at samples of [cin, h, w] and c classes."""
    f = 64 * down(down(down(h))) * down(down(down(w)))
    return f, 32 * cin * 25 + 3 * 32 + 32 * 32 * 25 + 3 * 32 + 64 * 32 * 25 + 3 * 64 + c * f + c


class GNLeNet(torch.nn.Module):
    """A locally built module with GN-LeNet's 14 parameter tensors in its registration order."""

    def __init__(self, cin=1, c=10, hw=(28, 28), groups=2):
        super().__init__()
        gn = torch.nn.GroupNorm
        self.features = torch.nn.Sequential(
            torch.nn.Conv2d(cin, 32, 5, padding=2), torch.nn.MaxPool2d(3, 2), gn(groups, 32),
            torch.nn.ReLU(),
            torch.nn.Conv2d(32, 32, 5, padding=2), gn(groups, 32), torch.nn.MaxPool2d(3, 2),
            torch.nn.ReLU(),
            torch.nn.Conv2d(32, 64, 5, padding=2), gn(groups, 64), torch.nn.MaxPool2d(3, 2),
            torch.nn.ReLU())
        self.classifier = torch.nn.Sequential(torch.nn.Linear(sizes(cin, hw[0], hw[1], c)[0], c))

    def forward(self, x, params):
        return F.log_softmax(self.classifier(torch.flatten(self.features(x), 1)), dim=1)


def perturb(model, gen, scale=0.2):
    """Biases and GroupNorm affines off their 0 / 1 defaults."""
    with torch.no_grad():
        for q in model.parameters():
            if q.dim() == 1:
                q.add_(scale * torch.randn(q.shape, generator=gen))
    return model


def forward_logits(theta, x, c, dtype=torch.float64):
    """The classifier's output z [M, C] of a flattened row `theta` on x [M, Cin, H, W], restated
    from torch.nn.functional in `dtype` (float64: the yardstick; float32: the arithmetic the
    reference uses, whose error against float64 is e32)."""
    cin, h, w = x.shape[1:]
    f, p = sizes(cin, h, w, c)
    assert theta.numel() == p
    t = theta.to(dtype)
    shapes = [(32, cin, 5, 5), (32,), (32,), (32,), (32, 32, 5, 5), (32,), (32,), (32,),
              (64, 32, 5, 5), (64,), (64,), (64,), (c, f), (c,)]
    ps, o = [], 0
    for s in shapes:
        n = int(np.prod(s))
        ps.append(t[o:o + n].reshape(s))
        o += n
    a = F.conv2d(x.to(dtype), ps[0], ps[1], padding=2)
    a = F.relu(F.group_norm(F.max_pool2d(a, 3, 2), 2, ps[2], ps[3], 1e-5))
    a = F.conv2d(a, ps[4], ps[5], padding=2)
    a = F.relu(F.max_pool2d(F.group_norm(a, 2, ps[6], ps[7], 1e-5), 3, 2))
    a = F.conv2d(a, ps[8], ps[9], padding=2)
    a = F.relu(F.max_pool2d(F.group_norm(a, 2, ps[10], ps[11], 1e-5), 3, 2))
    return F.linear(a.flatten(1), ps[12], ps[13])


def load_fixture(name):
    d = np.load(os.path.join(GOLDEN, "gn_lenet", name + ".npz"))
    return {k: d[k] for k in d.files}


@pytest.mark.parametrize("name", ["gn_lenet_mnist", "gn_lenet_cifar"])
def test_float64_forward_reproduces_the_reference(name):
    """The yardstick of the GPU tests against the reference's own fp32 log-probs: 1e-5 absolute."""
    d = load_fixture(name)
    cin, h, w, c = (int(v) for v in d["shape"])
    assert d["theta"].dtype == np.float32 and d["theta"].shape == (sizes(cin, h, w, c)[1],)
    assert d["theta"].shape[0] == {"gn_lenet_mnist": 80554, "gn_lenet_cifar": 85354}[name]
    assert d["x"].shape == (4, cin, h, w) and d["logprobs"].shape == (4, c)
    z = forward_logits(torch.from_numpy(d["theta"]), torch.from_numpy(d["x"]), c)
    err = float((F.log_softmax(z, 1) - torch.from_numpy(d["logprobs"]).double()).abs().max())
    print(f"{name}: max |float64 restatement - reference fp32 log-probs| = {err:.3g}")
    assert err <= 1e-5
    # the same from a locally built module holding the row: registration order and layer order
    mdl = GNLeNet(cin, c, (h, w))
    torch.nn.utils.vector_to_parameters(torch.from_numpy(d["theta"]), mdl.parameters())
    with torch.no_grad():
        lp = mdl.forward(torch.from_numpy(d["x"]), {})
    assert float((lp - torch.from_numpy(d["logprobs"])).abs().max()) <= 1e-5


def test_fixtures_perturb_every_bias_and_affine():
    from niidmix import family
    for name in ("gn_lenet_mnist", "gn_lenet_cifar"):
        d = load_fixture(name)
        cin, h, w, c = (int(v) for v in d["shape"])
        off = family.gn_lenet_offsets(cin, c, sizes(cin, h, w, c)[0])
        for i in (1, 2, 3, 5, 6, 7, 9, 10, 11, 13):
            v = d["theta"][off[i]:off[i + 1]]
            default = 1.0 if i in (2, 6, 10) else 0.0
            assert np.all(v != default) and np.abs(v - default).max() < 2.0, (name, i)


def test_gn_lenet_shape_and_offsets():
    from niidmix import family, ops
    for cin, c, hw, f, p in [(1, 10, (28, 28), 256, 80554), (1, 10, (24, 24), 256, 80554),
                             (3, 10, (32, 32), 576, 85354), (1, 3, (15, 15), 64, None),
                             (3, 10, (17, 15), 64, None)]:
        mdl = GNLeNet(cin, c, hw)
        assert family.gn_lenet_shape(mdl) == (cin, c, f)
        assert family.linear_shape(mdl) is None
        off = family.gn_lenet_offsets(cin, c, f)
        ps = list(mdl.parameters())
        assert len(off) == 15 and off[0] == 0
        assert [off[i + 1] - off[i] for i in range(14)] == [q.numel() for q in ps]
        assert off[-1] == sum(q.numel() for q in ps) == sizes(cin, hw[0], hw[1], c)[1]
        assert ops.gnlenet_sizes(cin, hw[0], hw[1], c) == (f, off[-1])
        if p is not None:
            assert off[-1] == p
    assert family.gn_lenet_shape(torch.nn.Linear(4, 3)) is None
    mdl = GNLeNet()
    mdl.features[2].weight.requires_grad_(False)
    assert family.gn_lenet_shape(mdl) is None                    # not trainable
    assert family.gn_lenet_shape(GNLeNet().double()) is None     # not fp32
    mdl = GNLeNet()
    mdl.features[4] = torch.nn.Conv2d(32, 32, 3, padding=1)
    assert family.gn_lenet_shape(mdl) is None                    # a 3 x 3 convolution
    mdl = GNLeNet()
    mdl.extra = torch.nn.Parameter(torch.ones(1))
    assert family.gn_lenet_shape(mdl) is None                    # a fifteenth tensor
    # the group count is not in the shapes: the forward probe's business (test_gpu_eval_gnlenet)
    assert family.gn_lenet_shape(GNLeNet(groups=4)) == (1, 10, 256)


class Net(torch.nn.Module):
    def __init__(self, k=784, c=10):
        super().__init__()
        self.fc = torch.nn.Linear(k, c)

    def forward(self, x, params):
        return F.log_softmax(self.fc(x.view(-1, self.fc.in_features)), dim=1)


def _params(**alg):
    a = {"learning-rate": 0.1, "learning-momentum": 0.0, "batch-size": 16, "initial-averaging": False,
         "clique-gradient": False, "unbiased-gradient": False, "device-evaluation": True}
    a.update(alg)
    return {"meta": {"log": "WARNING"}, "topology": {"name": "ring"}, "algorithm": a, "logger": {}}


def _nodes(params, models):
    from niidmix import d_sgd
    return [{"rank": r, "epoch": 0, "train-set": [(torch.zeros(1, 28, 28), 0)] * 4, "model": mdl,
             "optimizer": d_sgd.optimizer(mdl, params)} for r, mdl in enumerate(models)]


def test_all_gn_lenet_node_list_is_accepted():
    from niidmix import d_sgd, evaluate
    p = _params()
    nodes = _nodes(p, [GNLeNet(), GNLeNet()])
    assert evaluate.check_eligible(nodes, p) == (1, 10, 256)
    state, _, _ = d_sgd.init(nodes, {"edges": {}}, p)
    assert state["step"] == 0
    assert evaluate.check_eligible(_nodes(p, [Net(), Net()]), p) == (784, 10)     # as before


def test_mixed_and_misshapen_lists_are_refused():
    from niidmix import d_sgd, evaluate
    p = _params()
    for models in ([GNLeNet(), Net()], [Net(), GNLeNet()], [GNLeNet(), GNLeNet(c=9)],
                   [GNLeNet(), GNLeNet(hw=(32, 32))], [GNLeNet(), GNLeNet(cin=3)],
                   [GNLeNet(c=1025)], [GNLeNet(cin=5)]):
        with pytest.raises(ValueError, match="device-evaluation"):
            d_sgd.init(_nodes(p, models), {"edges": {}}, p)
    with pytest.raises(ValueError, match="device-evaluation"):
        evaluate.check_eligible(_nodes(p, [Net(c=1025)]), p)
    # --device-training with GN-LeNet stays refused
    p = _params(**{"device-training": True, "device-evaluation": False})
    with pytest.raises(ValueError, match="device-training"):
        d_sgd.init(_nodes(p, [GNLeNet(), GNLeNet()]), {"edges": {}}, p)


def test_wrong_sample_shape_is_refused():
    """A set's samples must be [Cin, H, W] images that give the classifier's F."""
    from niidmix import evaluate, family
    ev = evaluate.DeviceEvaluator(_params(), device="cpu")
    spec = (family.GN_LENET, (1, 10, 256))

    def st(shape, m=3):
        x = torch.zeros((m,) + shape)
        return evaluate._Set(x.reshape(m, -1), torch.zeros(m, dtype=torch.int32), 0, 0,
                             (x, torch.zeros(m, dtype=torch.int64)))
    assert ev._check(st((1, 28, 28)), spec, "the test set") == (1, 28, 28, 10)
    assert ev._check(st((1, 24, 24)), spec, "the test set") == (1, 24, 24, 10)
    assert ev._check(st((1, 24, 29)), spec, "the test set") == (1, 24, 29, 10)    # F = 256 as well
    for shape in ((784,), (28, 28), (1, 32, 32), (3, 28, 28), (1, 14, 28), (1, 65, 24)):
        with pytest.raises(ValueError, match="device-evaluation"):
            ev._check(st(shape), spec, "the test set")
    bad = st((1, 28, 28))
    bad.hi = 10
    with pytest.raises(ValueError, match="device-evaluation.*label"):
        ev._check(bad, spec, "the test set")
    assert ev._check(st((784,)), (family.LINEAR, (784, 10)), "the test set") == (784, 10)
    with pytest.raises(ValueError, match="device-evaluation"):
        ev._check(st((1, 28, 28)), (family.LINEAR, (783, 10)), "the test set")


def test_gnlenet_eval_argument_errors_without_gpu():
    """Validation happens before any HIP call, in the order include/niidmix.h documents; the
    made-up addresses are never dereferenced."""
    from niidmix import _lib
    L = _lib.lib
    Fn = L.niidmix_gnlenet_eval_rows_f32
    B = L.niidmix_gnlenet_eval_rows_scratch_bytes
    base, far, scr = 1 << 20, 1 << 30, 1 << 40
    n, ml = 2, 100
    p = 80554

    def call(theta=base, ld_t=None, data=8, labels=8, rows=8, start=8, length=8, n_jobs=n, max_len=ml,
             loss=far, correct=far + 4096, pred=None, ld_pred=0, logits=None, ld_logits=0, Cin=1,
             H=28, W=28, C=10, scratch=scr, nbytes=None):
        if ld_t is None:
            ld_t = p if (Cin, H, W, C) == (1, 28, 28, 10) else 1 << 24
        if nbytes is None:
            nbytes = B(max(n_jobs, 1), max(max_len, 0), Cin, H, W, C)
        return Fn(theta, ld_t, data, labels, rows, start, length, n_jobs, max_len, loss, correct, pred,
                  ld_pred, logits, ld_logits, Cin, H, W, C, scratch, nbytes, None)

    def err():
        return L.niidmix_last_error()

    for name in ("theta", "data", "labels", "rows", "start", "length", "loss", "correct", "scratch"):
        assert call(**{name: None}) == _lib.EINVAL and b"null" in err(), name
    for name in ("n_jobs", "Cin", "H", "W", "C"):
        for v in (0, -1):
            assert call(**{name: v}) == _lib.EINVAL and b">= 1" in err(), name
    assert call(max_len=-1) == _lib.EINVAL and b"max_len" in err()
    assert call(n_jobs=0, theta=None) == _lib.EINVAL and b"null" in err()          # null before sizes
    assert call(C=1025) == _lib.EUNSUPPORTED and b"C 1025" in err()
    assert call(Cin=5) == _lib.EUNSUPPORTED and b"Cin 5" in err()
    for hw in (14, 65, 1):
        assert call(H=hw) == _lib.EUNSUPPORTED and b"H" in err()
        assert call(W=hw) == _lib.EUNSUPPORTED
    assert call(H=0, C=1025) == _lib.EINVAL                                       # sizes before limits
    assert call(C=1025, ld_t=1) == _lib.EUNSUPPORTED                              # limits before ld
    assert call(ld_t=p - 1) == _lib.EINVAL and b"leading dimension < P" in err()
    assert call(pred=far + 8192, ld_pred=ml - 1) == _lib.EINVAL and b"ld_pred" in err()
    assert call(logits=far + (1 << 20), ld_logits=ml - 1) == _lib.EINVAL and b"ld_logits" in err()
    assert call(ld_t=p - 1, pred=far + 8192, ld_pred=ml - 1) == _lib.EINVAL and b"leading" in err()
    assert call(nbytes=1) == _lib.EINVAL and b"scratch" in err()
    assert call(scratch=scr + 4) == _lib.EINVAL and b"scratch" in err()           # 8-B alignment
    assert call(pred=far + 8192, ld_pred=ml - 1, nbytes=1) == _lib.EINVAL and b"ld_pred" in err()
    assert call(loss=base) == _lib.EALIAS and b"overlaps theta" in err()
    assert call(correct=base + 4 * (p - 1)) == _lib.EALIAS
    assert call(pred=base - 4 * ml, ld_pred=ml) == _lib.EALIAS                    # its second row
    assert call(logits=base - 4 * ml * 10, ld_logits=ml) == _lib.EALIAS           # its second job
    assert call(scratch=base + 8) == _lib.EALIAS
    assert call(loss=base, nbytes=1) == _lib.EINVAL                               # scratch before alias


def test_gnlenet_scratch_bytes_is_monotone():
    from niidmix import _lib
    B = _lib.lib.niidmix_gnlenet_eval_rows_scratch_bytes
    assert B(0, 10, 1, 28, 28, 10) == 0 and B(5, 0, 1, 28, 28, 10) == 0
    assert B(5, 10, 0, 28, 28, 10) == 0 and B(5, 10, 1, 14, 28, 10) == 0 and B(5, 10, 1, 28, 65, 10) == 0
    assert B(5, 10, 5, 28, 28, 10) == 0 and B(5, 10, 1, 28, 28, 1025) == 0
    assert B(1, 1, 1, 15, 15, 1) >= 12
    for hw in (15, 28, 32, 34, 35, 64):
        for n, m in [(1, 1), (7, 63), (7, 64), (1000, 10000), (3, 257)]:
            b = B(n, m, 3, hw, hw, 10)
            assert b % 16 == 0 and b >= 12 * n * ((m + 1) // 2)
            assert B(n + 1, m, 3, hw, hw, 10) >= b
            assert B(n, m + 1, 3, hw, hw, 10) >= b and B(n, m + 2, 3, hw, hw, 10) > b
            assert B(n, m, 3, hw, hw, 11) >= b and B(n, m, 3, hw + 1 if hw < 64 else hw, hw, 10) >= b
    # proportional to the jobs of one call, plus at most a constant (the activation slots of a
    # shape that does not fit in LDS)
    for hw in (32, 64):
        b1, b2 = B(1000, 10000, 3, hw, hw, 10), B(2000, 10000, 3, hw, hw, 10)
        assert b2 - b1 == 1000 * 5000 * 12


def test_header_declares_the_gnlenet_symbols_at_abi_6():
    from niidmix import _lib
    assert _lib.lib.niidmix_abi_version() == 6
    text = open(os.path.join(REPO, "include", "niidmix.h")).read()
    assert re.search(r"^int niidmix_gnlenet_eval_rows_f32\(", text, re.M)
    assert re.search(r"^int64_t niidmix_gnlenet_eval_rows_scratch_bytes\(", text, re.M)
    assert re.search(r"#define\s+NIIDMIX_ABI_VERSION\s+6\b", text)
    for word in ("fp32 FMAs only", "no floating-point atomics", "theta is not written",
                 "A job of length 0", "the same bits"):
        assert word in text
    assert "niidmix_gnlenet_eval_rows_f32" in _lib.SIGNATURES
    assert "niidmix_gnlenet_eval_rows_scratch_bytes" in _lib.SIGNATURES
