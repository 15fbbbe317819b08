"""--device-evaluation-mfma without a GPU: argument checks, scratch, tile rule, flag, routing."""
import json

import pytest

# (H, W) -> samples per tile: the minimum, the reference's, odd, the last of tile 4 and 2, beyond
TILES = {(15, 15): 4, (24, 24): 4, (28, 28): 4, (17, 15): 4, (28, 30): 4, (29, 29): 2, (32, 32): 2,
         (40, 36): 2, (42, 42): 2, (42, 43): 0, (44, 44): 0, (64, 64): 0, (44, 15): 4, (64, 15): 2}


def test_argument_errors_in_the_documented_order():
    """Before any HIP call (the made-up addresses are never dereferenced), in the existing entry
    point's order, the tighter limit with the other limits."""
    from niidmix import _lib
    L = _lib.lib
    B = L.niidmix_gnlenet_eval_rows_mfma_scratch_bytes
    base, far, scr, p, ml = 1 << 20, 1 << 30, 1 << 40, 80554, 100

    def call(theta=base, ld_t=p, n_jobs=2, max_len=ml, loss=far, pred=None, ld_pred=0, logits=None,
             ld_logits=0, Cin=1, H=28, W=28, C=10, scratch=scr, nbytes=None):
        if nbytes is None:
            nbytes = B(max(n_jobs, 1), max(max_len, 0), Cin, H, W, C)
        return L.niidmix_gnlenet_eval_rows_mfma_f32(theta, ld_t, 8, 8, 8, 8, 8, n_jobs, max_len, loss,
                                                    far + 4096, pred, ld_pred, logits, ld_logits, Cin, H,
                                                    W, C, scratch, nbytes, None)
    err = L.niidmix_last_error
    assert call(theta=None, n_jobs=0) == _lib.EINVAL and b"null" in err()           # null before sizes
    assert call(H=0, C=1025) == _lib.EINVAL and b">= 1" in err()                     # sizes before limits
    assert call(C=1025, H=44, W=44) == _lib.EUNSUPPORTED and b"C 1025" in err()
    assert call(H=65, ld_t=1 << 24) == _lib.EUNSUPPORTED and b"15 <= H" in err()
    assert call(H=44, W=44, ld_t=1) == _lib.EUNSUPPORTED and b"matrix-core" in err()  # limits before ld
    assert call(H=40, W=36, Cin=2, ld_t=1) == _lib.EINVAL and b"leading dimension < P" in err()
    assert call(pred=far + 8192, ld_pred=ml - 1, nbytes=1) == _lib.EINVAL and b"ld_pred" in err()
    assert call(logits=far + (1 << 20), ld_logits=ml - 1) == _lib.EINVAL and b"ld_logits" in err()
    assert call(loss=base, nbytes=1) == _lib.EINVAL and b"scratch" in err()         # scratch before alias
    assert call(loss=base) == _lib.EALIAS and b"overlaps theta" in err()


@pytest.mark.parametrize("hw", sorted(TILES))
def test_tile_rule_and_scratch_bytes(hw):
    """ops.gn_mfma_tile restates the library's rule: 12 B per (job, tile), monotone, 0 beyond."""
    from niidmix import _lib, ops
    B = _lib.lib.niidmix_gnlenet_eval_rows_mfma_scratch_bytes
    ts = ops.gn_mfma_tile(*hw)
    assert ts == TILES[hw]
    for n, m in [(1, 1), (7, 63), (7, 64), (1000, 10000), (3, 257)]:
        b = B(n, m, 3, *hw, 10)
        assert b == ((n * -(-m // ts) * 12 + 15) // 16 * 16 if ts else 0)
        assert B(n + 1, m, 3, *hw, 10) >= b and B(n, m + 1, 3, *hw, 10) >= b
        assert ts == 0 or B(n + 1, m + ts, 3, *hw, 10) > b


def test_flag_needs_device_evaluation_and_reaches_params(tmp_path, monkeypatch, capsys):
    from niidmix import d_sgd, evaluate
    monkeypatch.setattr(d_sgd, "load_topology", lambda rundir: {"edges": {}, "weights": []})
    run = tmp_path / "both"
    run.mkdir()
    (run / "params.json").write_text(json.dumps({"topology": {"name": "ring"}}))
    d_sgd.main(["--rundir", str(run), "--device-evaluation", "--device-evaluation-mfma"])
    params = json.loads((run / "params.json").read_text())
    assert params["algorithm"]["device-evaluation-mfma"] is True and evaluate.mfma_enabled(params)
    run = tmp_path / "alone"
    run.mkdir()
    (run / "params.json").write_text(json.dumps({"topology": {"name": "ring"}}))
    with pytest.raises(SystemExit):
        d_sgd.main(["--rundir", str(run), "--device-evaluation-mfma"])
    assert "--device-evaluation-mfma needs --device-evaluation" in capsys.readouterr().err
    with pytest.raises(ValueError, match="--device-evaluation-mfma needs --device-evaluation"):
        d_sgd.init([], {}, {"meta": {"log": "WARNING"}, "logger": {}, "topology": {"name": "ring"},
                            "algorithm": {"device-evaluation-mfma": True}})


def test_family_routing_rule(monkeypatch):
    """The new op exactly when flagged, the shape fits and its tile's class is measured faster."""
    from niidmix import _lib, family, ops
    fam, lib = family.GN_LENET, _lib.lib
    for hw, ts in TILES.items():
        sizes = (3, *hw, 10)
        want = bool(ts) and fam.MFMA_FASTER[ts]
        assert fam.mfma(sizes, True) == want and not fam.mfma(sizes, False)
        flagged, plain = fam.eval_plan(sizes, mfma=True), fam.eval_plan(sizes)
        assert flagged.kernel == ("k_gnl_eval_mfma" if want else "k_gnl_eval") and plain.kernel == "k_gnl_eval"
        assert flagged.op is (ops.gnlenet_eval_rows_mfma if want else ops.gnlenet_eval_rows)
        assert plain.op is ops.gnlenet_eval_rows
        old = lib.niidmix_gnlenet_eval_rows_scratch_bytes(5, 100, *sizes)
        new = lib.niidmix_gnlenet_eval_rows_mfma_scratch_bytes(5, 100, *sizes)
        assert plain.scratch_bytes(5, 100) == old
        assert flagged.scratch_bytes(5, 100) == (new if want else old)
    monkeypatch.setattr(fam, "MFMA_FASTER", {4: True, 2: False})      # a class measured slower
    assert fam.mfma((1, 28, 28, 10), True) and not fam.mfma((3, 32, 32, 10), True)
    assert fam.eval_plan((1, 28, 28, 10), mfma=True).kernel == "k_gnl_eval_mfma"      # read when made
    assert fam.eval_plan((3, 32, 32, 10), mfma=True).kernel == "k_gnl_eval"
