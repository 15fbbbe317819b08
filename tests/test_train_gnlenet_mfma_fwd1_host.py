"""--device-training-gn-lenet-mfma-fwd1 without a GPU: the flag, the C entry's answers, the family's rule."""
import itertools

import pytest

import test_train_gnlenet_host as tt
from test_train_gnlenet_mfma_host import BAD

KEYS = ["device-training-gn-lenet-mfma" + k for k in ("", "-sample", "-conv1", "-fwd1")]
NEEDS = "--device-training-gn-lenet-mfma-fwd1 needs --device-training-gn-lenet-mfma-conv1"


def _call(new, **bad):
    """(code, message) of the _mfma_conv1 or the new entry; made-up addresses, never read: every call fails a check."""
    from niidmix import _lib
    L = _lib.lib
    need = L.niidmix_gnlenet_nll_grad_rows_scratch_bytes(2, 5, 1, 28, 28, 10)
    a = dict(theta=1 << 20, ld_t=80554, data=8, labels=8, idx=8, length=8, b_max=5, rows=8, n_rows=2,
             grad=1 << 30, ld_g=80554, loss=1 << 36, Cin=1, H=28, W=28, C=10, scratch=1 << 40, nbytes=need)
    a.update(bad)
    a["nbytes"] = need - 1 if a["nbytes"] == -1 else a["nbytes"]
    fn = getattr(L, f"niidmix_gnlenet_nll_grad_rows_mfma_{'fwd1' if new else 'conv1'}_f32")
    return fn(*a.values(), None), L.niidmix_last_error()


def test_the_entry_answers_as_the_conv1_entry():
    """Also over the grid of shapes: a band of conv1's pass fits wherever the sample pass does."""
    from niidmix import _lib
    for bad, code in BAD:
        base = _call(False, **bad)
        assert base[0] == getattr(_lib, code) and _call(True, **bad) == base, bad
    big = dict(ld_t=1 << 20, ld_g=1 << 20, nbytes=8)
    for cin, h, w in itertools.product((1, 4), range(15, 65), range(15, 65)):
        base = _call(False, Cin=cin, H=h, W=w, **big)
        assert _call(True, Cin=cin, H=h, W=w, **big) == base, (cin, h, w)
    assert _call(True, Cin=4, H=42, W=42, **big)[0] == _lib.EINVAL != _call(True, H=43, W=43, **big)[0]


def test_the_flag_needs_its_base_flag(tmp_path, monkeypatch):
    from niidmix import d_sgd, train
    seen = {}
    monkeypatch.setattr(d_sgd.m, "rundir", lambda args: str(tmp_path))
    monkeypatch.setattr(d_sgd.m, "params", lambda rundir: {"topology": {"name": "ring"}})
    monkeypatch.setattr(d_sgd.m, "extend", lambda rundir, key, val: seen.update({key: val}))
    monkeypatch.setattr(d_sgd, "load_topology", lambda rundir: {})
    base = ["--rundir", str(tmp_path), "--device-training-gn-lenet"] + ["--" + k for k in KEYS[:2]]
    with pytest.raises(SystemExit):
        d_sgd.main(base + ["--" + KEYS[3]])
    d_sgd.main(base + ["--" + KEYS[2], "--" + KEYS[3]])
    assert all(seen["algorithm"][k] is True for k in KEYS)
    p = tt._params(**dict.fromkeys(KEYS[:2] + KEYS[3:], True))
    nodes = tt._nodes(p, [tt.th.GNLeNet(), tt.th.GNLeNet()])
    for refuse in (lambda: d_sgd.init(nodes, {"edges": {}}, p), lambda: train.check_eligible(nodes, p)):
        with pytest.raises(ValueError, match=NEEDS):
            refuse()
    p = tt._params(**dict.fromkeys(KEYS, True))
    assert train.gn_mfma_fwd1_enabled(p) and not train.gn_mfma_fwd1_enabled(tt._params())


@pytest.mark.parametrize("sizes,tile", [((1, 15, 15, 3), 4), ((1, 28, 28, 10), 4), ((3, 32, 32, 10), 2),
                                        ((4, 42, 41, 3), 2), ((1, 43, 43, 10), 0), ((4, 64, 64, 3), 0)])
def test_the_family_rule_follows_its_table(sizes, tile, monkeypatch):
    from niidmix import family, ops
    fam = family.GN_LENET
    for name in ("GRAD_MFMA_SAMPLE_FASTER", "GRAD_MFMA_CONV1_FASTER"):
        monkeypatch.setattr(family, name, {4: True, 2: True})
    today = {sw: fam.grad_plan(sizes, 5, False, *sw).op for sw in itertools.product((False, True), repeat=3)}
    for table in ({4: True, 2: False}, {4: False, 2: True}):
        monkeypatch.setattr(family, "GRAD_MFMA_FWD1_FASTER", table)
        for mfma, sample, conv1, flag in itertools.product((False, True), repeat=4):
            new = mfma and sample and conv1 and flag and table.get(tile, False)
            assert family.grad_mfma_fwd1(sizes, mfma, sample, conv1, flag) is new
            plan = fam.grad_plan(sizes, 5, False, mfma, sample, conv1, mfma_fwd1=flag)
            assert plan.op is (ops.gnlenet_nll_grad_rows_mfma_fwd1 if new else today[mfma, sample, conv1])
    monkeypatch.setattr(family, "GRAD_MFMA_CONV1_FASTER", {4: False, 2: False})     # the base op is not routed
    assert not family.grad_mfma_fwd1(sizes, True, True, True, True)
    assert family.LINEAR.grad_plan((784, 10), 5, mfma=True, mfma_sample=True, mfma_conv1=True,
                                   mfma_fwd1=True).op is ops.linear_nll_grad_rows
