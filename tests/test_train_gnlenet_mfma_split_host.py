"""--device-training-gn-lenet-mfma-split without a GPU: the flag, the C entry's answers and scratch, the family's rule."""
import itertools

import pytest

import test_train_gnlenet_host as tt
from test_train_gnlenet_mfma_host import BAD

KEYS = ["device-training-gn-lenet-mfma" + k for k in ("", "-sample", "-conv1", "-split")]
NEEDS = "--device-training-gn-lenet-mfma-split needs --device-training-gn-lenet-mfma-conv1"
SHAPE = (1, 28, 28, 10)


def _call(new, **bad):
    """(code, message) of the plain or the new entry; made-up addresses, never read: every call fails a check."""
    from niidmix import _lib
    L = _lib.lib
    a = dict(theta=1 << 20, ld_t=80554, data=8, labels=8, idx=8, length=8, b_max=5, rows=8, n_rows=2,
             grad=1 << 30, ld_g=80554, loss=1 << 36, Cin=1, H=28, W=28, C=10, scratch=1 << 40, nbytes=None)
    a.update(bad)
    need = (L.niidmix_gnlenet_nll_grad_rows_mfma_split_scratch_bytes if new
            else L.niidmix_gnlenet_nll_grad_rows_scratch_bytes)(2, a["b_max"], *SHAPE)
    a["nbytes"] = {None: need, -1: need - 1}.get(a["nbytes"], a["nbytes"])
    fn = L.niidmix_gnlenet_nll_grad_rows_mfma_split_f32 if new else L.niidmix_gnlenet_nll_grad_rows_f32
    return fn(*a.values(), None), L.niidmix_last_error()


def test_the_entry_answers_as_the_plain_entry_but_for_its_shapes_and_scratch():
    from niidmix import _lib
    L = _lib.lib
    for bad, code in BAD:
        plain = _call(False, **bad)
        assert plain[0] == getattr(_lib, code) and _call(True, **bad) == plain, bad
    big = dict(ld_t=1 << 20, ld_g=1 << 20, nbytes=8)
    assert _call(True, H=43, W=43, **big)[0] == _lib.EUNSUPPORTED
    assert L.niidmix_gnlenet_grad_split_chunk(1, 43, 43, 10) == 0
    assert _call(True, Cin=4, H=42, W=42, **big)[0] == _lib.EINVAL
    ch = L.niidmix_gnlenet_grad_split_chunk(*SHAPE)
    old, new = L.niidmix_gnlenet_nll_grad_rows_scratch_bytes, L.niidmix_gnlenet_nll_grad_rows_mfma_split_scratch_bytes
    assert ch > 0 and all(new(2, b, *SHAPE) == old(2, b, *SHAPE) > 0 for b in (1, ch))
    b = 2 * ch + 1                         # three chunks: the partials follow the slots
    assert new(2, b, *SHAPE) - old(2, b, *SHAPE) == 2 * 3 * (3 * 32 * 800 + 32 * SHAPE[0] * 25) * 4
    assert _call(True, b_max=b, nbytes=-1)[0] == _lib.EINVAL        # one byte short of the longer scratch
    # the overlap checks cover the partials: the slots end 8 bytes before grad
    assert _call(True, b_max=b, scratch=(1 << 30) - old(2, b, *SHAPE) - 8)[0] == _lib.EALIAS


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
    assert train.gn_mfma_split_enabled(tt._params(**dict.fromkeys(KEYS, True)))
    assert not train.gn_mfma_split_enabled(tt._params())


@pytest.mark.parametrize("sizes,tile", [((1, 15, 15, 3), 4), ((1, 28, 28, 10), 4), ((3, 32, 32, 10), 2),
                                        ((4, 42, 41, 3), 2), ((1, 43, 43, 10), 0), ((4, 64, 64, 3), 0)])
def test_the_family_rule_follows_its_table(sizes, tile, monkeypatch):
    from niidmix import _lib, family, ops
    fam, L = family.GN_LENET, _lib.lib
    assert set(family.GRAD_MFMA_SPLIT_FASTER) == {4, 2}
    for name in ("GRAD_MFMA_SAMPLE_FASTER", "GRAD_MFMA_CONV1_FASTER"):
        monkeypatch.setattr(family, name, {4: True, 2: True})
    today = {sw: fam.grad_plan(sizes, 5, False, *sw).op for sw in itertools.product((False, True), repeat=3)}
    for table in ({4: True, 2: False}, {4: False, 2: True}):
        monkeypatch.setattr(family, "GRAD_MFMA_SPLIT_FASTER", table)
        for mfma, sample, conv1, flag in itertools.product((False, True), repeat=4):
            new = mfma and sample and conv1 and flag and table.get(tile, False)
            assert family.grad_mfma_split(sizes, mfma, sample, conv1, flag) is new
            plan = fam.grad_plan(sizes, 100, False, mfma, sample, conv1, mfma_split=flag)
            assert plan.op is (ops.gnlenet_nll_grad_rows_mfma_split if new else today[mfma, sample, conv1])
            size = L.niidmix_gnlenet_nll_grad_rows_mfma_split_scratch_bytes if new \
                else L.niidmix_gnlenet_nll_grad_rows_scratch_bytes
            assert plan.scratch_bytes(3) == size(3, 100, *sizes)
    monkeypatch.setattr(family, "GRAD_MFMA_CONV1_FASTER", {4: False, 2: False})     # the base op is not routed
    assert not family.grad_mfma_split(sizes, True, True, True, True)
    assert family.LINEAR.grad_plan((784, 10), 5, mfma=True, mfma_sample=True, mfma_conv1=True,
                                   mfma_split=True).op is ops.linear_nll_grad_rows
