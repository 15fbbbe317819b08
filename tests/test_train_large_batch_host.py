"""--device-training-large-batch, the parts that need no GPU: the flag's refusals, what it lifts on
the training and on the sampling side (and that nothing moves without it), the CLI key, the sliced C
entry's argument checks (made-up addresses, never dereferenced), its scratch size and its slice."""
import json
import os
import re

import pytest

import test_sampling_host as sh
import test_train_host as th
from conftest import REPO

LARGE = "device-training-large-batch"
FLAG = "--" + LARGE
TOPO = {"edges": {}}


def _params(**alg):
    return th._params(**{LARGE: True, **alg})


def test_flag_refusals_name_the_flag():
    from niidmix import d_sgd, ops, train
    assert train.FLAG_LARGE == FLAG and ops.MAX_B_SLICED == 2 ** 20
    # without a training flag: check_eligible and d_sgd.init alike
    p = _params()
    del p["algorithm"]["device-training"]
    assert train.large_enabled(p) and not train.enabled(p)
    for call in (lambda: train.check_eligible(th._nodes(p), p, TOPO),
                 lambda: d_sgd.init(th._nodes(p), TOPO, p)):
        with pytest.raises(ValueError, match=rf"{FLAG} .*needs --device-training"):
            call()
    # with GN-LeNet's flag
    p = _params(**{"device-training-gn-lenet": True})
    with pytest.raises(ValueError, match=rf"{FLAG} is for linear models"):
        train.check_eligible(th._nodes(p), p, TOPO)
    # a batch beyond the sliced kernel's
    p = _params(**{"batch-size": ops.MAX_B_SLICED + 1})
    with pytest.raises(ValueError, match=rf"{FLAG}: batch-size = {ops.MAX_B_SLICED + 1} exceeds"):
        train.check_eligible(th._nodes(p), p, TOPO)
    p = _params(**{"batch-size": ops.MAX_B_SLICED})
    assert train.check_eligible(th._nodes(p), p, TOPO) == (6, 3)
    # on a sample run the flag goes with --device-training-sample
    p = sh.tsh._params(**{LARGE: True, "batch-size": ops.MAX_BC})
    assert train.check_eligible(sh.tsh._nodes(p), p, sh.tsh._topo()) == (6, 3)


def test_training_limit_with_and_without_the_flag():
    from niidmix import family, ops, train
    c = 3
    batch = ops.MAX_BC // c + 1                      # batch * C = MAX_BC + C - (MAX_BC % C) > MAX_BC
    assert batch * c > ops.MAX_BC
    p = _params(**{"batch-size": batch})
    assert train.check_eligible(th._nodes(p), p, TOPO) == (6, c)
    q = th._params(**{"batch-size": batch})
    with pytest.raises(ValueError, match=rf"--device-training: C = 3, batch-size \* C = {batch * c} exceed"):
        train.check_eligible(th._nodes(q), q, TOPO)
    # batch * C = MAX_BC + C exactly, on the family's own refusal (C = 4 divides MAX_BC)
    lin = family.LINEAR
    lin.limits((6, 4), FLAG, ops.MAX_BC // 4 + 1, True)
    lin.limits((6, 4), FLAG, ops.MAX_BC // 4 + 1, large=True)
    with pytest.raises(ValueError, match="exceed the kernel's limits"):
        lin.limits((6, 4), "--device-training", ops.MAX_BC // 4 + 1)
    with pytest.raises(ValueError, match="C = 1025"):
        lin.limits((6, 1025), FLAG, 4, True)         # the flag lifts no class limit
    # the sliced op exactly beyond MAX_BC, and only under the flag
    assert lin.sliced(ops.MAX_BC // 4 + 1, (6, 4), True)
    assert not lin.sliced(ops.MAX_BC // 4, (6, 4), True)
    assert not lin.sliced(ops.MAX_BC // 4 + 1, (6, 4), False)
    L = __import__("niidmix")._lib.lib
    assert lin.grad_scratch_bytes(2, 8192, (6, 4), True) == lin.grad_scratch_bytes(2, 8192, (6, 4)) == \
        4 * L.niidmix_linear_nll_grad_rows_scratch_elems(2, 8192, 4)
    assert lin.grad_scratch_bytes(2, 8193, (6, 4), True) == \
        4 * L.niidmix_linear_nll_grad_rows_sliced_scratch_elems(2, 8193, 6, 4)
    assert lin.cut is False


def test_sampling_limit_with_and_without_the_flag():
    from niidmix import ops, train
    most = ops.epoch_perm_max_len()
    for extra in ({}, {"device-training-sample": True}):
        p = sh._params(**{LARGE: True, "device-sampling-cached": True, "batch-size": 8193, **extra})
        assert train.check_eligible(sh.tsh._nodes(p), p, sh.tsh._topo()) == (6, 3)
    p = sh._params(**{LARGE: True, "device-sampling-cached": True, "batch-size": most})
    assert train.check_eligible(sh.tsh._nodes(p), p, sh.tsh._topo()) == (6, 3)
    p = sh._params(**{LARGE: True, "device-sampling-cached": True, "batch-size": most + 1})
    with pytest.raises(ValueError, match=rf"--device-sampling: batch size {most + 1} is not in 1..{most}"):
        train.check_eligible(sh.tsh._nodes(p), p, sh.tsh._topo())
    # plain --device-sampling keeps its cap, and says which flag lifts it
    p = sh._params(**{LARGE: True, "batch-size": 8193})
    with pytest.raises(ValueError, match=r"--device-sampling: batch size 8193 is not in 1\.\.8192.*"
                                         r"--device-sampling-cached"):
        train.check_eligible(sh.tsh._nodes(p), p, sh.tsh._topo())
    # without the flag the cached mode's cap is the parent's
    p = sh._params(**{"device-sampling-cached": True, "batch-size": 8193})
    with pytest.raises(ValueError, match=r"--device-sampling: batch size 8193 is not in 1\.\.8192, the "
                                         r"longest batch the kernel draws$"):
        train.check_eligible(sh.tsh._nodes(p), p, sh.tsh._topo())


def test_cli_flag_writes_its_key_and_needs_a_linear_training_flag(tmp_path, monkeypatch, capsys):
    from niidmix import d_sgd
    monkeypatch.setattr(d_sgd, "load_topology", lambda rundir: TOPO)
    for i, (argv, want) in enumerate(((["--device-training", FLAG], True),
                                      (["--device-training-sample", FLAG], True),
                                      (["--device-training"], None))):
        run = tmp_path / f"run{i}"
        run.mkdir()
        (run / "params.json").write_text(json.dumps({"topology": {"name": "ring"}}))
        d_sgd.main(["--rundir", str(run)] + argv)
        alg = json.loads((run / "params.json").read_text())["algorithm"]
        assert alg.get(LARGE) is want and alg.get("device-training") is True, argv
    for i, argv in enumerate(([FLAG], ["--device-training-gn-lenet", FLAG])):
        run = tmp_path / f"bad{i}"
        run.mkdir()
        (run / "params.json").write_text(json.dumps({"topology": {"name": "ring"}}))
        with pytest.raises(SystemExit):
            d_sgd.main(["--rundir", str(run)] + argv)
        assert FLAG + " needs" in capsys.readouterr().err
        assert "algorithm" not in json.loads((run / "params.json").read_text())


def test_sliced_argument_errors_without_gpu():
    """Validation happens before any HIP call, so the documented codes come back on a CPU-only
    host too (the made-up addresses are never dereferenced)."""
    from niidmix import _lib
    L = _lib.lib
    F = L.niidmix_linear_nll_grad_rows_sliced_f32
    E = L.niidmix_linear_nll_grad_rows_sliced_scratch_elems
    base, far, scr = 1 << 20, 1 << 30, 1 << 40
    k, c, b = 5, 3, 4
    p = c * k + c

    def call(theta=base, ld_t=p, data=8, labels=8, bidx=8, blen=8, b_max=b, rows=8, n_rows=2,
             grad=far, ld_g=p, loss=8, K=k, C=c, scratch=scr, elems=None):
        if elems is None:
            elems = E(n_rows, b_max, K, C)
        return F(theta, ld_t, data, labels, bidx, blen, b_max, rows, n_rows, grad, ld_g, loss, K, C,
                 scratch, elems, None)

    def err():
        return L.niidmix_last_error()

    for name in ("theta", "data", "labels", "bidx", "blen", "rows", "grad", "loss", "scratch"):
        assert call(**{name: None}) == _lib.EINVAL and b"null" in err(), name
    for name in ("n_rows", "b_max", "K", "C"):
        assert call(**{name: -1}, elems=0) == _lib.EINVAL and b"negative" in err(), name
    assert call(elems=-1) == _lib.EINVAL and b"negative" in err()
    assert call(n_rows=0, theta=None) == _lib.OK                                  # empty before null
    assert call(b_max=0, elems=0) == _lib.EINVAL and b">= 1" in err()
    assert call(C=1025, ld_t=1025 * k + 1025, ld_g=1025 * k + 1025, b_max=1, elems=1 << 40) == _lib.EUNSUPPORTED
    assert b"C 1025" in err()
    assert call(b_max=2 ** 20 + 1, elems=1 << 40) == _lib.EUNSUPPORTED and b"b_max" in err()
    assert call(K=2 ** 20 + 1, ld_t=1 << 40, ld_g=1 << 40, elems=1 << 40) == _lib.EUNSUPPORTED and b"K" in err()
    assert call(ld_t=p - 1, b_max=2 ** 20 + 1, elems=1 << 40) == _lib.EUNSUPPORTED  # limits before ld
    assert call(elems=1) == _lib.EINVAL and b"scratch" in err()                  # short scratch
    assert call(elems=E(2, b, k, c) - 1) == _lib.EINVAL and b"scratch" in err()
    assert call(ld_t=p - 1) == _lib.EINVAL and b"leading dimension < C * K + C" in err()
    assert call(ld_g=p - 1) == _lib.EINVAL and b"leading dimension < C * K + C" in err()
    assert call(grad=base) == _lib.EALIAS and b"theta and grad" in err()
    assert call(grad=base + 4 * (p + 2)) == _lib.EALIAS      # grad starts inside theta's 2nd row
    assert call(scratch=base + 4) == _lib.EALIAS and b"scratch" in err()
    # b_max * C = 32769, beyond the existing entry: past the limits, refused for its ld alone
    assert 10923 * 3 == 32769
    assert call(b_max=10923, ld_t=p - 1) == _lib.EINVAL and b"leading dimension" in err()
    G = L.niidmix_linear_nll_grad_rows_f32
    assert G(base, p - 1, 8, 8, 8, 8, 10923, 8, 2, far, p, 8, k, c, scr, 1 << 40, None) == _lib.EUNSUPPORTED
    # a scratch size beyond int64
    assert call(n_rows=1 << 40, b_max=2 ** 20, C=1024, K=2 ** 20, ld_t=1 << 31, ld_g=1 << 31,
                elems=(1 << 63) - 1) == _lib.EUNSUPPORTED and b"int64" in err()
    # (no call here passes every check: that one would launch on the made-up addresses)


def test_scratch_and_slice():
    from niidmix import _lib, ops
    L = _lib.lib
    E = L.niidmix_linear_nll_grad_rows_sliced_scratch_elems
    S = L.niidmix_linear_nll_grad_rows_sliced_slice
    for args in ((0, 4, 5, 3), (2, 0, 5, 3), (2, 4, 0, 3), (2, 4, 5, 0), (-1, 4, 5, 3), (2, -4, 5, 3)):
        assert E(*args) == 0, args
    for n_rows, k, c in ((1, 784, 10), (3, 6, 3), (1000, 784, 10), (2, 5, 1024)):
        sizes = [E(n_rows, b, k, c) for b in (1, 2, 7, 255, 256, 257, 3276, 3277, 12800, 2 ** 20)]
        assert all(a > 0 for a in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1], (n_rows, k, c)
        # at least the partial logits of the existing entry, one partial gradient row per (row, slice)
        # and one loss partial per (row, slice)
        b = 12800
        n_sl = -(-b // S(c))
        assert E(n_rows, b, k, c) >= L.niidmix_linear_nll_grad_rows_scratch_elems(n_rows, b, c) + \
            n_rows * n_sl * (c * k + c + 1)
    # the slice: a function of C alone whose dz fits the 32 KiB of LDS the kernel asks for, a power
    # of two, and more than one sample for every C the kernels hold
    assert S(0) == 0 and S(-3) == 0 and S(1025) == 0
    for c in range(1, 1025):
        s = S(c)
        assert 8 <= s <= 1024 and s & (s - 1) == 0 and s * c * 4 <= 32768, c
        assert s == 1024 or 2 * s * c * 4 > 32768, c                 # the largest such
        assert ops.linear_sliced_slice(c) == s
    assert S(10) == 512 and S(3) == 1024 and S(17) == 256 and S(1024) == 8
    text = open(os.path.join(REPO, "include", "niidmix.h")).read()
    assert "S * C * 4 <= 32768 bytes of LDS" in text


def test_header_library_and_ops_declare_the_new_names():
    import torch
    from niidmix import _lib, ops
    text = open(os.path.join(REPO, "include", "niidmix.h")).read()
    assert re.search(r"^int niidmix_linear_nll_grad_rows_sliced_f32\(const float \*theta,", text, re.M)
    assert re.search(r"^int64_t niidmix_linear_nll_grad_rows_sliced_slice\(int64_t C\);", text, re.M)
    assert re.search(r"^int64_t niidmix_linear_nll_grad_rows_sliced_scratch_elems\(int64_t n_rows, "
                     r"int64_t b_max, int64_t K,", text, re.M)
    assert "#define NIIDMIX_ABI_VERSION 6" in text and _lib.lib.niidmix_abi_version() == 6
    for name in ("niidmix_linear_nll_grad_rows_sliced_f32", "niidmix_linear_nll_grad_rows_sliced_slice",
                 "niidmix_linear_nll_grad_rows_sliced_scratch_elems"):
        assert name in _lib.SIGNATURES
    assert hasattr(torch.ops.niidmix, "linear_nll_grad_rows_sliced")
    assert callable(ops.linear_nll_grad_rows_sliced) and ops.MAX_BC == 32768
    # the op refuses CPU tensors as its neighbour does: no fallback
    z = torch.zeros
    with pytest.raises(RuntimeError):
        ops.linear_nll_grad_rows_sliced(z(1, 21), z(4, 6), z(4, dtype=torch.int32), z(1, 4, dtype=torch.int32),
                                        z(1, dtype=torch.int32), z(1, dtype=torch.int32), z(1, 21), z(1), 6, 3)
