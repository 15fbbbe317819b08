"""--device-training-gn-lenet-mfma-sample without a GPU: the flag, the C entry's answers, the family's rule."""
import pytest

import test_train_gnlenet_host as tt
from test_train_gnlenet_mfma_host import BAD

MFMA, KEY = "device-training-gn-lenet-mfma", "device-training-gn-lenet-mfma-sample"
NEEDS = "--device-training-gn-lenet-mfma-sample needs --device-training-gn-lenet-mfma"


def _call(new, **bad):
    """(code, message) of the plain or new entry; made-up addresses, never read: every call fails a check."""
    from niidmix import _lib
    L = _lib.lib
    need = L.niidmix_gnlenet_nll_grad_rows_scratch_bytes(2, 5, 1, 28, 28, 10)
    a = dict(theta=1 << 20, ld_t=80554, data=8, labels=8, idx=8, length=8, b_max=5, rows=8, n_rows=2,
             grad=1 << 30, ld_g=80554, loss=1 << 36, Cin=1, H=28, W=28, C=10, scratch=1 << 40, nbytes=need)
    a.update(bad)
    a["nbytes"] = need - 1 if a["nbytes"] == -1 else a["nbytes"]
    fn = L.niidmix_gnlenet_nll_grad_rows_mfma_sample_f32 if new else L.niidmix_gnlenet_nll_grad_rows_f32
    return fn(*a.values(), None), L.niidmix_last_error()


def test_the_entry_answers_as_the_plain_entry_but_for_its_shapes():
    """The other entries' bad calls and codes; 1 x 43 x 43 pools to 21 x 21: the plain entry's shape
    check passes (it stops at the scratch size given here), the new entry's does not; 42 x 42 passes."""
    from niidmix import _lib, ops
    for bad, code in BAD:
        plain = _call(False, **bad)
        assert plain[0] == getattr(_lib, code) and _call(True, **bad) == plain, bad
    big = dict(ld_t=1 << 20, ld_g=1 << 20, nbytes=8)
    assert ops.gn_mfma_tile(43, 43) == 0 and ops.gn_mfma_tile(42, 42) == 2
    assert _call(False, H=43, W=43, **big)[0] == _lib.EINVAL
    rc, err = _call(True, H=43, W=43, **big)
    assert rc == _lib.EUNSUPPORTED and b"sample pass" in err
    assert _call(True, H=42, W=42, **big)[0] == _lib.EINVAL
    assert _call(True, H=43, W=43, C=1025)[1].startswith(b"C 1025")            # C's refusal comes first
    B = _lib.lib.niidmix_gnlenet_nll_grad_rows_scratch_bytes        # the values before the new entry
    assert B(1000, 20, 3, 32, 32, 10) == 3922880000 and B(100, 128, 1, 28, 28, 10) == 1868390400


def test_the_flag_needs_its_base_flag(tmp_path, monkeypatch):
    from niidmix import d_sgd, train
    seen = {}
    monkeypatch.setattr(d_sgd.m, "rundir", lambda args: str(tmp_path))
    monkeypatch.setattr(d_sgd.m, "params", lambda rundir: {"topology": {"name": "ring"}})
    monkeypatch.setattr(d_sgd.m, "extend", lambda rundir, key, val: seen.update({key: val}))
    monkeypatch.setattr(d_sgd, "load_topology", lambda rundir: {})
    base = ["--rundir", str(tmp_path), "--device-training-gn-lenet"]
    with pytest.raises(SystemExit):
        d_sgd.main(base + ["--device-training-gn-lenet-mfma-sample"])
    d_sgd.main(base + ["--device-training-gn-lenet-mfma", "--device-training-gn-lenet-mfma-sample"])
    assert seen["algorithm"][KEY] is True and seen["algorithm"][MFMA] is True
    p = tt._params(**{KEY: True})
    nodes = tt._nodes(p, [tt.th.GNLeNet(), tt.th.GNLeNet()])
    for refuse in (lambda: d_sgd.init(nodes, {"edges": {}}, p), lambda: train.check_eligible(nodes, p)):
        with pytest.raises(ValueError, match=NEEDS):
            refuse()
    p = tt._params(**{MFMA: True, KEY: True})
    assert train.check_eligible(tt._nodes(p, [tt.th.GNLeNet(), tt.th.GNLeNet()]), p) == (1, 10, 256)


@pytest.mark.parametrize("sizes,tile", [((1, 15, 15, 3), 4), ((1, 28, 28, 10), 4), ((3, 32, 32, 10), 2),
                                        ((4, 42, 41, 3), 2), ((1, 43, 43, 10), 0), ((4, 64, 64, 3), 0)])
def test_the_family_rule_follows_its_table(sizes, tile, monkeypatch):
    from niidmix import family, ops
    fam = family.GN_LENET
    assert ops.gn_mfma_tile(sizes[1], sizes[2]) == tile and set(family.GRAD_MFMA_SAMPLE_FASTER) == {4, 2}
    today = {m: fam.grad_plan(sizes, 5, mfma=m).op for m in (False, True)}
    for table in ({4: True, 2: False}, {4: False, 2: True}):
        monkeypatch.setattr(family, "GRAD_MFMA_SAMPLE_FASTER", table)
        for mfma in (False, True):
            for flag in (False, True):
                new = mfma and flag and table.get(tile, False)
                assert family.grad_mfma_sample(sizes, mfma, flag) is new
                plan = fam.grad_plan(sizes, 5, False, mfma, flag)
                assert plan.op is (ops.gnlenet_nll_grad_rows_mfma_sample if new else today[mfma])
    assert family.LINEAR.grad_plan((784, 10), 5, mfma=True, mfma_sample=True).op is ops.linear_nll_grad_rows
