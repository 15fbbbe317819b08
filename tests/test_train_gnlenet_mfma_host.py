"""--device-training-gn-lenet-mfma without a GPU: the C entry answers bad calls as the plain entry
does, the flag needs its base flag, niidmix.family's rule picks the op its table says."""
import pytest

import test_train_gnlenet_host as tt

KEY = "device-training-gn-lenet-mfma"
BAD = [(dict(theta=None), "EINVAL"), (dict(loss=None, n_rows=0), "EINVAL"), (dict(n_rows=0), "EINVAL"),
       (dict(b_max=-1, H=14), "EINVAL"), (dict(H=14), "EUNSUPPORTED"), (dict(W=65), "EUNSUPPORTED"),
       (dict(H=65, ld_t=1), "EUNSUPPORTED"), (dict(ld_t=80553, nbytes=1), "EINVAL"),
       (dict(ld_g=80553), "EINVAL"), (dict(nbytes=-1, grad=1 << 20), "EINVAL"),
       (dict(scratch=(1 << 40) + 4), "EINVAL"), (dict(grad=1 << 20), "EALIAS"),
       (dict(loss=(1 << 20) + 4 * 80554), "EALIAS"), (dict(scratch=(1 << 30) + 8), "EALIAS")]


@pytest.mark.parametrize("bad,code", BAD, ids=[",".join(b) for b, _ in BAD])
def test_the_entry_answers_as_the_plain_entry(bad, code):
    """(what is wrong, the plain entry's code) in the header's order; made-up addresses, never read."""
    from niidmix import _lib
    L = _lib.lib
    need = L.niidmix_gnlenet_nll_grad_rows_scratch_bytes(2, 5, 1, 28, 28, 10)
    a = dict(theta=1 << 20, ld_t=80554, data=8, labels=8, idx=8, length=8, b_max=5, rows=8, n_rows=2,
             grad=1 << 30, ld_g=80554, loss=1 << 36, Cin=1, H=28, W=28, C=10, scratch=1 << 40, nbytes=need)
    a.update(bad)
    a["nbytes"] = need - 1 if a["nbytes"] == -1 else a["nbytes"]
    got = [(fn(*a.values(), None), L.niidmix_last_error())
           for fn in (L.niidmix_gnlenet_nll_grad_rows_f32, L.niidmix_gnlenet_nll_grad_rows_mfma_f32)]
    assert got[0][0] == getattr(_lib, code) and got[1] == got[0]


def test_the_flag_needs_its_base_flag(tmp_path, monkeypatch):
    from niidmix import d_sgd, train
    seen = {}
    monkeypatch.setattr(d_sgd.m, "rundir", lambda args: str(tmp_path))
    monkeypatch.setattr(d_sgd.m, "params", lambda rundir: {"topology": {"name": "ring"}})
    monkeypatch.setattr(d_sgd.m, "extend", lambda rundir, key, val: seen.update({key: val}))
    monkeypatch.setattr(d_sgd, "load_topology", lambda rundir: {})
    with pytest.raises(SystemExit):
        d_sgd.main(["--rundir", str(tmp_path), "--device-training-gn-lenet-mfma"])
    d_sgd.main(["--rundir", str(tmp_path), "--device-training-gn-lenet", "--device-training-gn-lenet-mfma"])
    assert seen["algorithm"][KEY] is True and seen["algorithm"][tt.GN] is True
    p = tt._params(**{tt.GN: False, "device-training": False, KEY: True})
    nodes = tt._nodes(p, [tt.th.GNLeNet(), tt.th.GNLeNet()])
    with pytest.raises(ValueError, match="--device-training-gn-lenet-mfma needs --device-training-gn-lenet"):
        d_sgd.init(nodes, {"edges": {}}, p)
    p = tt._params(**{KEY: True})
    assert train.check_eligible(tt._nodes(p, [tt.th.GNLeNet(), tt.th.GNLeNet()]), p) == (1, 10, 256)


@pytest.mark.parametrize("sizes,cls", [((1, 15, 15, 3), "map"), ((1, 28, 28, 10), "map"),
                                       ((3, 32, 32, 10), "map"), ((3, 35, 32, 10), "bands"),
                                       ((2, 40, 36, 4), "bands"), ((4, 64, 64, 3), "bands")])
def test_the_family_rule_follows_its_table(sizes, cls, monkeypatch):
    import torch
    from niidmix import family, ops
    fam = family.GN_LENET
    assert fam.grad_mfma_class(sizes) == cls and set(fam.GRAD_MFMA_FASTER) == {"map", "bands"}
    b = 5
    bi = torch.zeros(2, b, dtype=torch.int32)
    for table in ({"map": True, "bands": False}, {"map": False, "bands": True}):
        monkeypatch.setattr(fam, "GRAD_MFMA_FASTER", table)
        assert fam.grad_mfma(sizes, True) is table[cls] and fam.grad_mfma(sizes, False) is False
        called = []
        monkeypatch.setattr(ops, "gnlenet_nll_grad_rows_mfma", lambda *a: called.append(("mfma",) + a[8:]))
        monkeypatch.setattr(ops, "gnlenet_nll_grad_rows", lambda *a: called.append(("plain",) + a[8:]))
        flagged, plain = fam.grad_plan(sizes, b, mfma=True), fam.grad_plan(sizes, b)
        assert flagged.op is (ops.gnlenet_nll_grad_rows_mfma if table[cls] else ops.gnlenet_nll_grad_rows)
        assert plain.op is ops.gnlenet_nll_grad_rows
        flagged(None, None, None, bi, *[None] * 4)
        plain(None, None, None, bi, *[None] * 4)
        assert called == [("mfma" if table[cls] else "plain",) + sizes, ("plain",) + sizes]
