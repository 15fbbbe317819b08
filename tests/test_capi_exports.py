"""The C-ABI library builds for gfx950, loads, and exports every symbol include/niidmix.h declares
(no compute calls: this runs without a GPU)."""
import ctypes
import os
import re

from conftest import REPO


def _declared_symbols():
    text = open(os.path.join(REPO, "include", "niidmix.h")).read()
    return sorted(set(re.findall(r"^\s*(?:int64_t|int|const char \*|void \*|void)\s*(niidmix_\w+)\s*\(",
                                 text, re.M)))


def test_header_declares_expected_api():
    syms = _declared_symbols()
    for s in ["niidmix_abi_version", "niidmix_last_error", "niidmix_mix_csr_f32",
              "niidmix_mix_clique_f32", "niidmix_mix_dense_f32", "niidmix_mean_rows_f32",
              "niidmix_mix_tile_lds_f32", "niidmix_grad_segment_mean_f32", "niidmix_hbm_alloc",
              "niidmix_hbm_free"]:
        assert s in syms


def test_library_exports_every_declared_symbol():
    from niidmix import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in _declared_symbols():
        assert hasattr(lib, s), s
    assert set(_lib.SIGNATURES) == set(_declared_symbols())
    assert _lib.lib.niidmix_abi_version() == _lib.ABI_VERSION


def test_library_is_gfx950_code_object():
    from niidmix import _lib
    data = open(_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in data


def test_argument_errors_without_gpu():
    """Validation happens before any HIP call, so errors are reported on a CPU-only host too."""
    from niidmix import _lib
    L = _lib.lib
    rc = L.niidmix_mix_csr_f32(None, 4, None, 4, 1, 4, None, None, None, 0, None)
    assert rc == _lib.EINVAL and b"null" in L.niidmix_last_error()
    rc = L.niidmix_mix_csr_f32(16, 4, 16, 4, 1, 4, 8, 8, 8, 0, None)
    assert rc == _lib.EALIAS
    rc = L.niidmix_mix_csr_f32(16, 4, 1024, 4, 1, 4, 8, 8, 8, 16, None)
    assert rc == _lib.EINVAL        # unknown mode
    rc = L.niidmix_mix_csr_f32(16, 4, 1024, 4, 1, 4, 8, 8, 8, 2 | 8, None)
    assert rc == _lib.EINVAL        # AVERAGE_ONLY and MEAN are exclusive
    rc = L.niidmix_mix_csr_f32(16, 2, 1024, 4, 1, 4, 8, 8, 8, 0, None)
    assert rc == _lib.EINVAL        # ld < p
    assert L.niidmix_mix_csr_f32(16, 4, 1024, 4, 0, 4, 8, 8, 8, 0, None) == _lib.OK  # empty
    plan = _lib.CliquePlanC(1, 4, 5, 4, 0, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8)
    rc = L.niidmix_mix_clique_f32(16, 4, 1024, 4, 4, ctypes.byref(plan), None)
    assert rc == _lib.EUNSUPPORTED   # n_groups 5
    plan = _lib.CliquePlanC(1, 300, 2, 300, -1, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8)
    rc = L.niidmix_mix_clique_f32(16, 4, 1 << 24, 4, 4, ctypes.byref(plan), None)
    assert rc == _lib.EINVAL         # negative max_clique_res
    plan = _lib.CliquePlanC(1, 4, 1, 4, 0, 8, 8, 8, 8, 8, 8, 8, 8, None, 8, 8)
    rc = L.niidmix_mix_clique_f32(16, 4, 1024, 4, 4, ctypes.byref(plan), None)
    assert rc == _lib.EINVAL         # the CSR (non-finite guard) is required
    # partial overlap of x and y over the member rows (Jacobi): 4 rows of ld 8 floats
    plan = _lib.CliquePlanC(1, 4, 1, 4, 0, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8)
    base = 1 << 20
    rc = L.niidmix_mix_clique_f32(base, 8, base + 4 * 20, 8, 8, ctypes.byref(plan), None)
    assert rc == _lib.EALIAS         # y starts inside x's 3rd row
    rc = L.niidmix_mix_clique_blocked_f32(base, base + 4 * 1024 * 2, 8, 1024, 1024, 8192, 8192,
                                          ctypes.byref(plan), None)
    assert rc == _lib.EALIAS         # y inside x's member rows of block 0
    rc = L.niidmix_mix_csr_f32(base + 4 * 20, 8, base, 8, 4, 8, 8, 8, 8, 0, None)
    assert rc == _lib.EALIAS         # x starts inside y
    rc = L.niidmix_mix_dense_f32(16, 4, 1024, 4, 4, 4, 8, None, 8, 8, None)
    assert rc == _lib.EINVAL         # dense: the CSR (non-finite guard) is required
    # ABI 5: the bf16x6 dense GEMM and its W split
    assert L.niidmix_dense_split_elems(1000) == 3 * 1024 * 1008
    assert L.niidmix_dense_split_elems(0) == 0
    rc = L.niidmix_mix_dense_bf16x6_f32(16, 4, 1024, 4, 4, 4, 16, None, 8, 8, None)
    assert rc == _lib.EINVAL         # the CSR (non-finite guard) is required
    rc = L.niidmix_mix_dense_bf16x6_f32(16, 4, 1024, 4, 4, 4, 8, 8, 8, 8, None)
    assert rc == _lib.EUNSUPPORTED   # split W must be 16-B aligned
    rc = L.niidmix_mix_dense_bf16x6_f32(base, 8, base + 4 * 20, 8, 4, 8, 1 << 24, 8, 8, 8, None)
    assert rc == _lib.EALIAS
    rc = L.niidmix_dense_split_w(4096, 4, 4096 + 16, None)
    assert rc == _lib.EALIAS         # w and its split overlap
    # the bf16x6 GEMM's 32-bit offsets -- 16 rows of ld_x (ld_x >= 2^25) or a split
    # W of 2^31 B (n = 19 000) -- are refused, never launched (niidmix.ops.b6_fits avoids them)
    ld = 1 << 25
    rc = L.niidmix_mix_dense_bf16x6_f32(base, ld, base + 4 * 4 * ld, ld, 4, 8, 1 << 24, 8, 8, 8, None)
    assert rc == _lib.EUNSUPPORTED
    rc = L.niidmix_mix_dense_bf16x6_f32(base, 8, base + 4 * 8 * 19000, 8, 19000, 8, 1 << 24, 8, 8, 8,
                                        None)
    assert rc == _lib.EUNSUPPORTED
    tp = _lib.TilePlanC(1, 12, 0, 8, 8, 8, 8, 8, 8)
    rc = L.niidmix_mix_tile_f32(16, 4, 1024, 4, 1, 4, ctypes.byref(tp), 0, None)
    assert rc == _lib.EUNSUPPORTED   # tile height 12
    tp = _lib.TilePlanC(1, 16, 0, None, 8, 8, 8, 8, 8)
    rc = L.niidmix_mix_tile_f32(16, 4, 1024, 4, 1, 4, ctypes.byref(tp), 0, None)
    assert rc == _lib.EINVAL         # null sub_ptr
    tp = _lib.TilePlanC(1, 16, 0, 8, 8, 8, 8, 8, 8)
    assert L.niidmix_mix_tile_f32(16, 4, 1024, 4, 1, 4, ctypes.byref(tp), 9, None) == _lib.EINVAL
    assert L.niidmix_mix_tile_f32(16, 4, 16, 4, 1, 4, ctypes.byref(tp), 0, None) == _lib.EALIAS
    # ABI 3: partial overlaps are caught over the full [n_rows, ld] extents (4 rows of ld 8)
    assert L.niidmix_mix_tile_f32(base, 8, base + 4 * 20, 8, 4, 8, ctypes.byref(tp), 0, None) == _lib.EALIAS
    lp = _lib.TileLdsPlanC(1, 16, 1, 8, 1, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8)   # seg*/mf* NULL
    assert L.niidmix_mix_tile_lds_f32(base, 8, base + 4 * 20, 8, 4, 8, ctypes.byref(lp), 0, None) == _lib.EALIAS
    G = L.niidmix_grad_segment_mean_f32
    assert G(None, 4, 16, 4, 1, 4, 1, 8, 8, None) == _lib.EINVAL
    assert G(16, 4, 16, 4, 1, 4, 1, 8, 8, None) == _lib.EALIAS
    assert G(16, 2, 1024, 4, 1, 4, 1, 8, 8, None) == _lib.EINVAL
    assert G(16, 4, 1024, 4, 1, 4, 0, 8, 8, None) == _lib.OK
    assert G(base, 8, base + 4 * 20, 8, 4, 8, 1, 8, 8, None) == _lib.EALIAS   # partial overlap
    B = L.niidmix_grad_segment_mean_blocked_f32
    assert B(None, 1024, 1, 4, 1024, 1024, 4096, 4096, 1, 8, 8, None) == _lib.EINVAL    # null
    assert B(16, 1024, 1, 4, 1024, 1000, 4096, 4096, 1, 8, 8, None) == _lib.EINVAL      # block_cols
    assert B(16, 1024, 1, 4, 1024, 1024, 512, 4096, 1, 8, 8, None) == _lib.EINVAL       # stride
    assert B(16, 16, 1, 4, 1024, 1024, 4096, 4096, 1, 8, 8, None) == _lib.EALIAS
    assert B(16, 1 << 30, 1, 6, 1024, 1024, 4096, 4096, 1, 8, 8, None) == _lib.EUNSUPPORTED  # p % 4
    assert B(16, 1024, 1, 4, 1024, 1024, 4096, 4096, 0, 8, 8, None) == _lib.OK         # empty
    # y with a LARGER block stride than g: g's 2 blocks at base + 8 KB, y's block 1 at base + 12 KB
    assert B(base + 8192, base, 1, 2048, 1024, 1024, 1024, 3072, 1, 8, 8, None) == _lib.EALIAS
    U = L.niidmix_update_rows_f32
    assert U(None, 4, 1024, 4, 1, 4, 8, None) == _lib.EINVAL
    assert U(base, 8, 1 << 30, 8, 4, 8, base + 4 * 20, None) == _lib.EALIAS   # avg inside x
    assert U(base, 8, base + 4 * 20, 8, 4, 8, 1 << 30, None) == _lib.EALIAS   # partial x / y overlap
    assert U(base, 8, base, 8, 0, 8, 8, None) == _lib.OK                       # no rows
    rc = L.niidmix_copy2d_async(None, 4, None, 4, 4, 1, 0, None)
    assert rc == _lib.EINVAL
    assert L.niidmix_stream_copy_f32(16, 1024, 6, None) == _lib.EUNSUPPORTED   # n % 4
    assert L.niidmix_stream_copy_f32(16, 32, 8, None) == _lib.EALIAS
    assert L.niidmix_stream_copy_f32(None, 32, 8, None) == _lib.EINVAL
    assert L.niidmix_stream_copy_f32(16, 1024, 0, None) == _lib.OK
    h = ctypes.c_void_p()
    assert L.niidmix_sharded_create(0, None, ctypes.byref(h)) == _lib.EINVAL and not h.value
    assert L.niidmix_sharded_destroy(None) == _lib.OK
    assert L.niidmix_mix_sharded_f32(None, None, 4, 0) == _lib.EINVAL
    E = L.niidmix_mix_ell_f32
    assert E(16, 4, 1024, 4, 1, 4, 9, 8, 8, 8, 0, None) == _lib.EUNSUPPORTED            # width 9
    assert E(16, 4, 1024, 4, 1, 4, 4, 8, 8, 8, 0, None) == _lib.EINVAL                  # unpadded width
    assert E(16, 4, 16, 4, 1, 4, 3, 8, 8, 8, 0, None) == _lib.EALIAS
    assert E(None, 4, 1024, 4, 1, 4, 3, 8, 8, 8, 0, None) == _lib.EINVAL
    S = L.niidmix_mix_strip_f32
    assert S(16, 64, 1 << 30, 64, 2, 64, 4, 8, 8, 8, 0, None) == _lib.EUNSUPPORTED     # ELL width 4
    assert S(16, 64, 1 << 30, 64, 257, 64, 3, 8, 8, 8, 0, None) == _lib.EUNSUPPORTED   # > 256 rows
    assert S(16, 64, 16 + 4 * 64, 64, 2, 64, 3, 8, 8, 8, 0, None) == _lib.EALIAS       # y = x's row 1
    assert S(None, 64, 1 << 30, 64, 2, 64, 3, 8, 8, 8, 0, None) == _lib.EINVAL
    assert S(16, 32, 1 << 30, 64, 2, 64, 3, 8, 8, 8, 0, None) == _lib.EINVAL          # ld_x < p
    assert S(18, 64, 1 << 30, 64, 2, 64, 3, 8, 8, 8, 0, None) == _lib.EUNSUPPORTED     # x not 4-B aligned
    assert S(16, 64, 1 << 30, 64, 2, 64, 3, 8, 8, 8, 16, None) == _lib.EINVAL         # unknown mode
    assert S(16, 64, 1 << 30, 64, 0, 64, 3, 8, 8, 8, 0, None) == _lib.OK              # no rows

    # ------------------------------------------------------------------------------------------
    # Order of the checks: calls with two things wrong return the code of the EARLIER check, and
    # "empty means OK" sits where each entry point has it.  Every call below is refused before any
    # HIP call (or is empty), so the made-up addresses are never dereferenced.
    AVG, LOW, MEAN = 2, 4, 8
    far = 1 << 30

    def err():
        return L.niidmix_last_error()

    C = L.niidmix_mix_csr_f32
    assert C(16, 4, far, 4, -1, 4, 8, 8, 8, 16, None) == _lib.EINVAL and b"negative" in err()
    assert C(16, 4, far, 4, 0, 4, 8, 8, 8, 16, None) == _lib.EINVAL and b"unknown mode" in err()
    assert C(16, 4, far, 4, 0, 4, 8, 8, 8, AVG | MEAN | 16, None) == _lib.EINVAL and b"exclusive" in err()
    assert C(16, 4, far, 4, 0, 4, 8, 8, 8, AVG | MEAN, None) == _lib.EINVAL    # flags before empty
    for m in (LOW, MEAN, AVG | LOW, LOW | MEAN | 1):
        assert C(None, 4, None, 4, 0, 4, None, None, None, m, None) == _lib.OK  # empty before null
    assert C(None, 4, None, 4, 1, 0, None, None, None, 0, None) == _lib.OK
    assert C(None, 2, 16, 4, 1, 4, 8, 8, 8, 0, None) == _lib.EINVAL and b"null" in err()
    assert C(16, 2, 16, 4, 1, 4, 8, 8, 8, 0, None) == _lib.EINVAL and b"leading" in err()  # ld before alias

    assert E(16, 4, far, 4, 0, 4, 3, 8, 8, 8, AVG | LOW, None) == _lib.OK
    assert E(16, 4, far, 4, 0, 4, 3, 8, 8, 8, MEAN, None) == _lib.EINVAL       # ell refuses MEAN
    assert E(16, 4, far, 4, 0, 4, 9, 8, 8, 8, 0, None) == _lib.EUNSUPPORTED    # width before empty
    assert E(16, 4, far, 4, 1, 0, 0, 8, 8, 8, 0, None) == _lib.EUNSUPPORTED
    assert E(16, 4, far, 4, 1, 4, 9, 8, 8, 8, MEAN, None) == _lib.EINVAL       # mode before width
    assert E(16, 4, far, 4, -1, 4, 9, 8, 8, 8, 0, None) == _lib.EINVAL         # negative before width
    assert E(None, 4, far, 4, 1, 4, 9, 8, 8, 8, 0, None) == _lib.EUNSUPPORTED  # width before null
    assert E(None, 4, far, 4, 0, 4, 8, None, None, None, 1, None) == _lib.OK
    assert E(16, 2, 16, 4, 1, 4, 3, 8, 8, 8, 0, None) == _lib.EINVAL           # ld before alias
    assert E(16, 4, 16, 4, 1, 4, 4, 8, 8, 8, 0, None) == _lib.EALIAS           # alias before padding
    assert E(16, 4, far, 4, 1, 4, 7, 8, 8, 8, 0, None) == _lib.EINVAL and b"pad the rows" in err()

    Bd = L.niidmix_mix_band_f32
    assert Bd(16, 4, far, 4, 0, 4, 3, 2, 8, 8, 8, 0, None) == _lib.EUNSUPPORTED    # (k, band) before empty
    assert Bd(16, 4, far, 4, 0, 4, 4, 1, 8, 8, 8, 0, None) == _lib.EUNSUPPORTED
    assert Bd(16, 4, far, 4, 0, 4, 3, 2, 8, 8, 8, MEAN, None) == _lib.EINVAL       # mode before (k, band)
    assert Bd(16, 4, far, 4, -1, 4, 3, 2, 8, 8, 8, 0, None) == _lib.EINVAL and b"negative" in err()
    assert Bd(None, 4, None, 4, 0, 4, 3, 1, None, None, None, AVG | LOW, None) == _lib.OK
    assert Bd(None, 4, None, 4, 5, 0, 5, 2, None, None, None, 1, None) == _lib.OK
    assert Bd(None, 4, far, 4, 2, 4, 3, 1, 8, 8, 8, 0, None) == _lib.EUNSUPPORTED  # rows before null
    assert Bd(None, 4, far, 4, 4, 4, 5, 2, 8, 8, 8, 0, None) == _lib.EUNSUPPORTED
    assert Bd(None, 4, far, 4, 3, 4, 3, 1, 8, 8, 8, 0, None) == _lib.EINVAL and b"null" in err()
    assert Bd(16, 4, far, 4, 3, 4, 3, 1, 8, 8, None, 0, None) == _lib.EINVAL
    assert Bd(16, 2, 16, 4, 3, 4, 3, 1, 8, 8, 8, 0, None) == _lib.EINVAL           # ld before alias
    assert Bd(16, 4, 16, 4, 3, 4, 3, 1, 8, 8, 8, 0, None) == _lib.EALIAS
    assert Bd(20, 4, 20, 4, 3, 4, 3, 1, 8, 8, 8, 0, None) == _lib.EALIAS           # alias before width
    assert Bd(base, 8, base + 4 * 20, 8, 5, 8, 5, 2, 8, 8, 8, 0, None) == _lib.EALIAS
    assert Bd(20, 4, far, 4, 3, 4, 3, 1, 8, 8, 8, 0, None) == _lib.EUNSUPPORTED    # 4-B aligned x
    assert Bd(16, 4, far + 4, 4, 3, 4, 3, 1, 8, 8, 8, 0, None) == _lib.EUNSUPPORTED
    assert Bd(16, 4, far, 4, 3, 3, 3, 1, 8, 8, 8, 0, None) == _lib.EUNSUPPORTED    # odd p
    assert Bd(16, 5, far, 6, 3, 4, 3, 1, 8, 8, 8, 1, None) == _lib.EUNSUPPORTED and b"even" in err()

    assert S(16, 64, far, 64, 0, 64, 4, 8, 8, 8, 0, None) == _lib.EUNSUPPORTED    # width before empty
    assert S(16, 64, far, 64, 2, 64, 4, 8, 8, 8, MEAN, None) == _lib.EINVAL       # mode before width
    assert S(None, 64, None, 64, 2, 0, 8, None, None, None, AVG | LOW | 1, None) == _lib.OK
    assert S(None, 64, far, 64, 257, 64, 3, 8, 8, 8, 0, None) == _lib.EUNSUPPORTED  # rows before null
    assert S(16, 32, 16, 64, 2, 64, 3, 8, 8, 8, 0, None) == _lib.EINVAL           # ld before alias
    assert S(18, 64, 18 + 4 * 64, 64, 2, 64, 5, 8, 8, 8, 0, None) == _lib.EALIAS  # alias before alignment

    T = L.niidmix_mix_tile_f32
    assert T(16, 4, far, 4, 1, 4, None, 0, None) == _lib.EINVAL and b"null plan" in err()
    tp0 = _lib.TilePlanC(0, 16, 0, None, None, None, None, None, None)
    assert T(None, 4, None, 4, 1, 4, ctypes.byref(tp0), AVG | 1, None) == _lib.OK
    assert T(None, 4, None, 4, 1, 4, ctypes.byref(tp0), LOW, None) == _lib.EINVAL  # tile: AVERAGE_ONLY only
    assert T(None, 4, None, 4, 1, 0, ctypes.byref(tp), 0, None) == _lib.OK
    tp12 = _lib.TilePlanC(0, 12, 0, 8, 8, 8, 8, 8, 8)
    assert T(16, 4, far, 4, 1, 4, ctypes.byref(tp12), 0, None) == _lib.EUNSUPPORTED  # height before empty
    assert T(16, 4, far, 4, 1, 4, ctypes.byref(tp12), LOW, None) == _lib.EINVAL      # mode before height
    assert T(16, 4, far, 4, 1, -1, ctypes.byref(tp12), 0, None) == _lib.EINVAL       # negative before height
    tpn = _lib.TilePlanC(-1, 12, 0, 8, 8, 8, 8, 8, 8)
    assert T(16, 4, far, 4, 1, 4, ctypes.byref(tpn), 0, None) == _lib.EINVAL
    assert T(None, 4, far, 4, 1, 4, ctypes.byref(tp), 0, None) == _lib.EINVAL and b"null pointer" in err()
    assert T(16, 2, 16, 4, 1, 4, ctypes.byref(tp), 0, None) == _lib.EINVAL and b"leading" in err()
    assert T(16, 4, 16, 4, 0, 4, ctypes.byref(tp), 0, None) == _lib.EINVAL and b"n_rows" in err()
    assert T(16, 4, far, 4, 0, 4, ctypes.byref(tp), 0, None) == _lib.EINVAL

    TL = L.niidmix_mix_tile_lds_f32

    def lds_plan(rt=16, n_grp=1, max_src=8, max_tiles=1, seg_ptr=None, seg=None, seg_w=None,
                 mf_ptr=None, mf=None, rem_rows=None, rem_regs=0, sub_ptr=8):
        return ctypes.byref(_lib.TileLdsPlanC(1, rt, n_grp, max_src, max_tiles, sub_ptr, 8, 8, 8, 8, 8,
                                              8, 8, 8, 8, seg_ptr, seg, seg_w, mf_ptr, mf, rem_rows,
                                              rem_regs))

    assert TL(base, 8, far, 8, 4, 8, None, 0, None) == _lib.EINVAL and b"null plan" in err()
    assert TL(base, 8, far, 8, 4, 8, lds_plan(), LOW, None) == _lib.EINVAL        # AVERAGE_ONLY only
    assert TL(base, 8, far, 8, 4, 8, lds_plan(rt=12), LOW, None) == _lib.EINVAL   # mode before height
    assert TL(base, 8, far, 8, 4, 8, lds_plan(rt=12, n_grp=0), 0, None) == _lib.EUNSUPPORTED
    assert TL(base, 8, far, 8, 4, -2, lds_plan(rt=12), 0, None) == _lib.EINVAL    # negative before height
    assert TL(base, 8, far, 8, 4, 8, lds_plan(n_grp=-1), 0, None) == _lib.EINVAL
    assert TL(None, 8, None, 8, 4, 8, lds_plan(n_grp=0), AVG, None) == _lib.OK
    assert TL(None, 8, None, 8, 4, 0, lds_plan(rt=32), 1, None) == _lib.OK
    assert TL(None, 8, far, 8, 4, 8, lds_plan(), 0, None) == _lib.EINVAL and b"null pointer" in err()
    assert TL(base, 8, far, 8, 4, 8, lds_plan(sub_ptr=None), 0, None) == _lib.EINVAL
    assert TL(base, 4, base, 8, 4, 8, lds_plan(), 0, None) == _lib.EINVAL and b"leading" in err()
    assert TL(base, 1 << 30, far * 64, 8, 0, 8, lds_plan(), 0, None) == _lib.EUNSUPPORTED  # ld_x before n_rows
    assert TL(base, 8, base, 8, 0, 8, lds_plan(), 0, None) == _lib.EINVAL and b"n_rows" in err()
    assert TL(base, 8, base + 4 * 20, 8, 4, 8, lds_plan(max_src=0), 0, None) == _lib.EALIAS
    assert TL(base, 8, far, 8, 4, 8, lds_plan(max_src=0), 0, None) == _lib.EUNSUPPORTED
    assert TL(base, 8, far, 8, 4, 8, lds_plan(max_src=257), 0, None) == _lib.EUNSUPPORTED
    assert TL(base, 8, far, 8, 4, 8, lds_plan(max_tiles=0), 0, None) == _lib.EUNSUPPORTED
    assert TL(base, 8, far, 8, 4, 8, lds_plan(max_tiles=13), 0, None) == _lib.EUNSUPPORTED
    assert TL(base, 8, far, 8, 4, 8, lds_plan(rt=32, max_tiles=5), 0, None) == _lib.EUNSUPPORTED
    assert TL(base, 8, far, 8, 4, 8, lds_plan(rt=8, max_tiles=17), 0, None) == _lib.EUNSUPPORTED
    assert TL(base, 8, far, 8, 4, 7, lds_plan(), 0, None) == _lib.EUNSUPPORTED and b"even" in err()
    assert TL(base, 9, far, 10, 4, 8, lds_plan(), 0, None) == _lib.EUNSUPPORTED
    assert TL(base + 4, 8, far, 8, 4, 8, lds_plan(), 0, None) == _lib.EUNSUPPORTED
    assert TL(base, 8, far + 4, 8, 4, 8, lds_plan(), 0, None) == _lib.EUNSUPPORTED
    # odd p before the segment-array checks
    assert TL(base, 8, far, 8, 4, 7, lds_plan(seg_ptr=8), 0, None) == _lib.EUNSUPPORTED
    assert TL(base, 8, far, 8, 4, 8, lds_plan(seg_ptr=8), 0, None) == _lib.EINVAL and b"segment" in err()
    assert TL(base, 8, far, 8, 4, 8, lds_plan(seg_ptr=8, seg=8), 1, None) == _lib.EINVAL
    assert TL(base, 8, far, 8, 4, 8, lds_plan(rem_rows=8), 0, None) == _lib.EINVAL and b"rem_rows" in err()
    assert TL(base, 8, far, 8, 4, 8, lds_plan(rt=8, seg_ptr=8, rem_rows=8), 0, None) == _lib.EINVAL
    assert TL(base, 8, far, 8, 4, 8, lds_plan(seg_ptr=8, seg=8, seg_w=8, mf_ptr=8, mf=8, rem_rows=8),
              0, None) == _lib.EINVAL
    assert TL(base, 8, far, 8, 4, 8, lds_plan(seg_ptr=8, seg=8, seg_w=8, rem_rows=8, rem_regs=5),
              1, None) == _lib.EINVAL and b"rem_regs" in err()
    assert TL(base, 8, far, 8, 4, 8, lds_plan(seg_ptr=8, seg=8, seg_w=8, mf_ptr=8), 0, None) == _lib.EINVAL
    assert b"MFMA" in err()

    Q = L.niidmix_mix_clique_f32
    QB = L.niidmix_mix_clique_blocked_f32

    def clique_plan(n_cliques=1, n_members=4, n_groups=1, max_clique=4, max_clique_res=0, **null):
        names = [f[0] for f in _lib.CliquePlanC._fields_[5:]]
        return ctypes.byref(_lib.CliquePlanC(n_cliques, n_members, n_groups, max_clique, max_clique_res,
                                             *[None if null.get(n) else 8 for n in names]))

    for rc in (Q(base, 8, far, 8, 8, None, None), QB(base, far, 8, 1024, 1024, 8192, 8192, None, None)):
        assert rc == _lib.EINVAL and b"null plan" in err()
    for kw in ({"n_cliques": -1}, {"n_members": -1}):
        assert Q(base, 8, far, 8, 8, clique_plan(**kw), None) == _lib.EINVAL and b"negative" in err()
        assert QB(base, far, 8, 1024, 1024, 8192, 8192, clique_plan(**kw), None) == _lib.EINVAL
        assert b"negative" in err()
    assert Q(base, 8, far, 8, -1, clique_plan(n_cliques=0), None) == _lib.EINVAL    # negative before empty
    assert QB(base, far, -1, 1024, 1024, 8192, 8192, clique_plan(n_cliques=0), None) == _lib.EINVAL
    assert Q(None, 2, None, 2, 8, clique_plan(n_cliques=0, csr_ptr=True), None) == _lib.OK  # empty before null
    assert Q(None, 2, None, 2, 0, clique_plan(coef=True), None) == _lib.OK
    assert QB(None, None, 8, 8, 1000, 4, 4, clique_plan(n_cliques=0, coef=True), None) == _lib.OK
    assert QB(None, None, 0, 8, 1000, 4, 4, clique_plan(), None) == _lib.OK
    for nm in ("clique_ptr", "member_row", "member_group", "coef", "res_ptr", "res_col", "res_val",
               "res_member", "csr_ptr", "csr_col", "csr_val"):
        assert Q(base, 8, far, 8, 8, clique_plan(**{nm: True}), None) == _lib.EINVAL and b"null pointer" in err()
        assert QB(base, far, 8, 1024, 1024, 8192, 8192, clique_plan(**{nm: True}), None) == _lib.EINVAL
        assert b"null pointer" in err()
    assert Q(None, 4, base, 8, 8, clique_plan(), None) == _lib.EINVAL and b"null pointer" in err()  # null before ld
    assert Q(base, 4, base, 8, 8, clique_plan(), None) == _lib.EINVAL and b"leading" in err()   # ld before alias
    assert Q(base, 8, base + 4 * 20, 8, 8, clique_plan(max_clique_res=-1), None) == _lib.EALIAS  # alias before res
    assert Q(base, 8, far, 8, 8, clique_plan(max_clique_res=-1), None) == _lib.EINVAL
    # no members: the extents are those of one row
    assert Q(base, 8, base + 4 * 4, 8, 8, clique_plan(n_members=0), None) == _lib.EALIAS
    assert Q(base, 8, far, 8, 6, clique_plan(), None) == _lib.EUNSUPPORTED           # p % 4
    assert Q(base + 8, 8, far, 8, 8, clique_plan(), None) == _lib.EUNSUPPORTED       # 8-B aligned x
    assert Q(base, 8, far, 8, 8, clique_plan(n_members=4096, n_groups=5, max_clique=100), None) == _lib.EUNSUPPORTED
    assert QB(None, far, 8, 1024, 1000, 8192, 8192, clique_plan(), None) == _lib.EINVAL and b"null pointer" in err()
    assert QB(base, base, 8, 1024, 1000, 8192, 8192, clique_plan(), None) == _lib.EINVAL   # block_cols before alias
    assert b"block_cols 1000: a power of two >= 64" in err()
    assert QB(base, far, 8, 1024, 32, 8192, 8192, clique_plan(), None) == _lib.EINVAL
    assert QB(base, far, 8, 1024, 128, 8192, 8192, clique_plan(max_clique=200), None) == _lib.EINVAL
    assert b">= 256" in err()
    assert QB(base, far, 8, 1024, 16, 8192, 8192, clique_plan(max_clique=300), None) == _lib.EINVAL
    assert b">= 32" in err()
    assert QB(base, base, 8, 512, 1024, 8192, 8192, clique_plan(), None) == _lib.EINVAL and b"row stride < block_cols" in err()
    assert QB(base, base, 8, 1024, 1024, 512, 8192, clique_plan(), None) == _lib.EINVAL and b"block stride" in err()
    assert QB(base, base, 8, 1024, 1024, 8192, 512, clique_plan(), None) == _lib.EINVAL
    assert QB(base, base + 4 * 1024 * 2, 8, 1024, 1024, 8192, 8192, clique_plan(max_clique=2000), None) == _lib.EALIAS
    # y with a larger block stride than x: x's 2 blocks at base + 8 KB, y's block 1 at base + 12 KB
    assert QB(base + 8192, base, 2048, 1024, 1024, 1024, 3072, clique_plan(n_members=1), None) == _lib.EALIAS
    assert QB(base, far, 8, 1024, 1024, 8192, 8192, clique_plan(max_clique=2000, max_clique_res=-1), None) == _lib.EUNSUPPORTED
    assert b"1024 members" in err()
    assert QB(base, far, 8, 1024, 1024, 8192, 8192, clique_plan(max_clique_res=-1), None) == _lib.EINVAL
    assert QB(base, far, 8, 1026, 1024, 8192, 8192, clique_plan(), None) == _lib.EUNSUPPORTED   # ld % 4
    assert QB(base, far, 8, 1024, 1024, 8192, 8194, clique_plan(), None) == _lib.EUNSUPPORTED
    assert QB(base + 4, far, 8, 1024, 1024, 8192, 8192, clique_plan(), None) == _lib.EUNSUPPORTED

    D = L.niidmix_mix_dense_f32
    D6 = L.niidmix_mix_dense_bf16x6_f32
    for fn, w in ((D, 8), (D6, 16)):
        assert fn(16, 4, far, 4, -1, 4, w, 8, 8, 8, None) == _lib.EINVAL and b"negative" in err()
        assert fn(None, 4, None, 4, 0, 4, None, None, None, None, None) == _lib.OK
        assert fn(None, 4, None, 4, 4, 0, None, None, None, None, None) == _lib.OK
        assert fn(16, 4, far, 4, 4, 4, None, 8, 8, 8, None) == _lib.EINVAL and b"null" in err()
        assert fn(16, 2, 16, 4, 4, 4, w, 8, 8, 8, None) == _lib.EINVAL and b"leading" in err()
        assert fn(base, 8, base + 4 * 20, 8, 4, 8, w, 8, 8, 8, None) == _lib.EALIAS
    assert D6(base, 8, base + 4 * 20, 8, 4, 8, 8, 8, 8, 8, None) == _lib.EUNSUPPORTED   # wp before alias
    assert D6(base, 4, base + 4 * 20, 8, 4, 8, 8, 8, 8, 8, None) == _lib.EINVAL         # ld before wp
    SW = L.niidmix_dense_split_w
    assert SW(4096, -1, 4096, None) == _lib.EINVAL
    assert SW(None, 0, None, None) == _lib.OK
    assert SW(4096, 4, None, None) == _lib.EINVAL
    assert SW(4096, 4, 4096 + 8, None) == _lib.EUNSUPPORTED                             # wp before alias

    M = L.niidmix_mean_rows_f32
    assert M(16, 4, -1, 4, far, None, AVG, None) == _lib.EINVAL and b"negative" in err()
    for m in (AVG, LOW, MEAN, 16):
        assert M(16, 4, 0, 4, far, None, m, None) == _lib.EINVAL and b"unknown mode" in err()  # no flags
    assert M(None, 4, 0, 4, None, None, 0, None) == _lib.OK
    assert M(None, 4, 4, 0, None, None, 1, None) == _lib.OK
    assert M(None, 4, 4, 4, far, None, 0, None) == _lib.EINVAL and b"null" in err()
    assert M(16, 4, 4, 4, None, None, 0, None) == _lib.EINVAL
    assert M(base, 4, 4, 8, base + 4 * 8, None, 0, None) == _lib.EINVAL and b"leading" in err()  # ld before alias
    assert M(base, 8, 4, 8, base + 4 * 20, None, 0, None) == _lib.EALIAS and b"mean overlaps x" in err()
    assert M(base, 8, 4, 8, base - 4 * 4, None, 1, None) == _lib.EALIAS

    assert G(16, 4, far, 4, -1, 4, 1, 8, 8, None) == _lib.EINVAL and b"negative" in err()
    assert G(None, 4, None, 4, 0, 4, 1, None, None, None) == _lib.OK                   # empty before null
    assert G(None, 4, None, 4, 1, 0, 1, None, None, None) == _lib.OK
    assert G(16, 4, far, 4, 1, 4, 1, None, 8, None) == _lib.EINVAL
    assert G(16, 2, 16, 4, 1, 4, 1, 8, 8, None) == _lib.EINVAL and b"leading" in err()  # ld before alias
    assert G(16, 4, 16, 4, 1, 4, 1, 8, 8, None) == _lib.EALIAS and b"g and y overlap" in err()
    assert B(16, 1024, -1, 4, 1024, 1000, 4096, 4096, 1, 8, 8, None) == _lib.EINVAL and b"negative" in err()
    assert B(None, None, 0, 4, 1024, 1000, 4096, 4096, 1, None, None, None) == _lib.OK  # empty first
    assert B(None, 1024, 1, 4, 1024, 1000, 4096, 4096, 1, 8, 8, None) == _lib.EINVAL and b"null" in err()
    assert B(16, 16, 1, 4, 1024, 512, 4096, 4096, 1, 8, 8, None) == _lib.EINVAL        # block_cols before alias
    assert b"block_cols 512: a power of two >= 1024" in err()
    assert B(16, 16, 1, 4, 512, 1024, 4096, 4096, 1, 8, 8, None) == _lib.EINVAL and b"row stride" in err()
    assert B(16, 16, 1, 4, 1024, 1024, 4096, 512, 1, 8, 8, None) == _lib.EINVAL and b"row stride" in err()
    assert B(16, 16, 1, 6, 1024, 1024, 4096, 4096, 1, 8, 8, None) == _lib.EALIAS       # alias before p % 4
    assert B(20, 20, 1, 4, 1026, 1024, 4096, 4096, 1, 8, 8, None) == _lib.EALIAS
    assert B(20, far, 1, 4, 1024, 1024, 4096, 4096, 1, 8, 8, None) == _lib.EUNSUPPORTED  # 4-B aligned g
    assert B(16, far, 1, 4, 1026, 1024, 4096, 4096, 1, 8, 8, None) == _lib.EUNSUPPORTED
    assert B(16, far, 1, 4, 1024, 1024, 4096, 4098, 1, 8, 8, None) == _lib.EUNSUPPORTED

    SG = L.niidmix_sgd_step_rows_f32
    assert SG(16, 4, far, 4, -1, 8, 1, 0.5, None) == _lib.EINVAL and b"negative" in err()
    assert SG(16, 4, far, 4, 4, 8, -1, 0.5, None) == _lib.EINVAL
    assert SG(None, 4, None, 4, 0, None, 1, 0.5, None) == _lib.OK                      # empty before null
    assert SG(None, 4, None, 4, 4, None, 0, 0.5, None) == _lib.OK
    for args in ((None, 4, far, 4, 4, 8), (16, 4, None, 4, 4, 8), (16, 4, far, 4, 4, None)):
        assert SG(*args, 1, 0.5, None) == _lib.EINVAL and b"null" in err()
    assert SG(None, 2, far, 4, 4, 8, 1, 0.5, None) == _lib.EINVAL and b"null" in err()  # null before ld
    assert SG(16, 2, far, 4, 4, 8, 1, 0.5, None) == _lib.EINVAL and b"leading dimension < ncols" in err()
    assert SG(16, 4, far, 2, 4, 8, 1, 0.5, None) == _lib.EINVAL
    MS = L.niidmix_sgd_momentum_step_rows_f32
    far2 = 1 << 31
    assert MS(16, 4, far, 4, far2, 4, -1, 8, 1, 0.5, 0.9, 0, None) == _lib.EINVAL and b"negative" in err()
    assert MS(16, 4, far, 4, far2, 4, 4, 8, -1, 0.5, 0.9, 0, None) == _lib.EINVAL
    assert MS(None, 4, None, 4, None, 4, 0, None, 1, 0.5, 0.9, 1, None) == _lib.OK      # empty before null
    assert MS(None, 4, None, 4, None, 4, 4, None, 0, 0.5, 0.9, 0, None) == _lib.OK
    assert MS(16, 4, far, 4, None, 4, 4, 8, 1, 0.5, 0.9, 0, None) == _lib.EINVAL and b"null" in err()
    assert MS(16, 4, far, 4, far2, 4, 4, None, 1, 0.5, 0.9, 0, None) == _lib.EINVAL
    assert MS(16, 4, 16, 4, far2, 2, 4, 8, 1, 0.5, 0.9, 0, None) == _lib.EINVAL         # ld before alias
    assert b"leading dimension < ncols" in err()
    assert MS(base, 8, base + 4 * 20, 8, far2, 8, 8, 8, 4, 0.5, 0.9, 0, None) == _lib.EALIAS
    assert b"p and g" in err()
    assert MS(base, 8, far, 8, base + 4 * 20, 8, 8, 8, 4, 0.5, 0.9, 1, None) == _lib.EALIAS
    assert b"p and buf" in err()
    assert MS(far, 8, base, 8, base + 4 * 20, 8, 8, 8, 4, 0.5, 0.9, 0, None) == _lib.EALIAS
    assert b"g and buf" in err()
    assert MS(base, 8, base, 8, base, 8, 8, 8, 4, 0.5, 0.9, 0, None) == _lib.EALIAS and b"p and g" in err()

    assert U(16, 4, far, 4, -1, 4, 8, None) == _lib.EINVAL and b"negative" in err()
    assert U(None, 4, None, 4, 4, 0, None, None) == _lib.OK
    assert U(16, 4, far, 4, 1, 4, None, None) == _lib.EINVAL and b"null" in err()
    assert U(base, 4, base + 4 * 20, 8, 4, 8, far, None) == _lib.EINVAL and b"leading" in err()  # ld before alias
    assert U(base, 8, base, 16, 4, 8, far, None) == _lib.EALIAS and b"same slab" in err()
    assert U(base, 8, base, 8, 4, 8, base + 4 * 20, None) == _lib.EALIAS and b"avg" in err()    # in place, avg inside
    assert U(base, 8, far, 8, 4, 8, far + 4 * 20, None) == _lib.EALIAS and b"avg" in err()      # avg inside y


def test_kernel_for_respects_bf16x6_limits():
    """Mixer.kernel_for('fast') picks the bf16x6 GEMM ('dense') for a dense W only
    within its limits (niidmix.ops.b6_fits: split W and 16 rows of the slab under 2^31 B), else the
    fp32 MFMA GEMM ('dense-f32'), which has none.  Host arithmetic only."""
    import numpy as np
    import torch
    from niidmix import ops
    n = 64
    w = np.random.default_rng(0).random((n, n)).astype(np.float32)
    w /= w.sum(0, keepdims=True)
    rp = np.arange(n + 1, dtype=np.int64) * n
    col = np.concatenate([[i] + [j for j in range(n) if j != i] for i in range(n)]).astype(np.int32)
    m = ops.Mixer(csr=ops.csr_from_numpy(rp, col, w[col, np.repeat(np.arange(n), n)]), device="cpu")
    assert m.kernel_for("fast") == "dense"
    ok = torch.empty_strided((2, 8), ((1 << 25) - 64, 1), device="meta")
    wide = torch.empty_strided((2, 8), (1 << 25, 1), device="meta")
    assert m.kernel_for("fast", ok) == "dense"
    assert m.kernel_for("fast", wide) == "dense-f32"
    assert m.kernel_for("fast", ok, wide) == "dense"        # y is addressed in 64 bits
    assert ops.b6_fits(18000) and not ops.b6_fits(19000)
