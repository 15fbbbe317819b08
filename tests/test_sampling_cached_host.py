"""--device-sampling-cached, the parts that need no GPU: the flag and its refusals, the CLI key,
the declarations of the four new C names under ABI 6, the argument checks of both C entries (made-up
addresses, never dereferenced) and SamplerState's record of which epoch's permutation the device
cache holds."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import test_sampling_host as sh
import test_train_sample_host as tsh
from conftest import REPO

SEED = sh.SEED


def _params(**alg):
    return sh._params(**{"device-sampling-cached": True, **alg})


def test_long_train_sets_are_accepted_under_the_flag_only():
    from niidmix import ops, train
    short, most = ops.draw_batches_max_len(), ops.epoch_perm_max_len()
    assert short == 8192 and most >= 2 ** 20
    p = _params()
    assert train.cached_enabled(p) and train.sampling_enabled(p)
    nodes = tsh._nodes(p)
    nodes[3]["train-set"] = range(short + 1)     # a range stands in for the samples: only len() is read
    assert train.check_eligible(nodes, p, tsh._topo()) == (6, 3)
    nodes[3]["train-set"] = range(most)
    assert train.check_eligible(nodes, p, tsh._topo()) == (6, 3)
    # above the new limit: refused, naming the flag
    nodes[3]["train-set"] = range(most + 1)
    with pytest.raises(ValueError, match=rf"--device-sampling-cached: node 3's train-set has {most + 1} samples"):
        train.check_eligible(nodes, p, tsh._topo())
    # without the flag the parent's refusal, word for word
    q = sh._params()
    nodes = tsh._nodes(q)
    nodes[3]["train-set"] = range(short + 1)
    with pytest.raises(ValueError, match=rf"--device-sampling: node 3's train-set has {short + 1} samples, "
                                         rf"the kernel sorts at most {short} per node"):
        train.check_eligible(nodes, q, tsh._topo())
    # the batch size stays bounded by the index block's kernel
    q = _params(**{"batch-size": short + 1})
    with pytest.raises(ValueError, match=rf"--device-sampling: batch size {short + 1}"):
        train.check_eligible(tsh._nodes(q), q, tsh._topo())


def test_flag_needs_device_sampling_and_a_training_flag():
    from niidmix import d_sgd, train
    q = _params()
    del q["algorithm"]["device-sampling"]
    for call in (lambda: train.check_eligible(tsh._nodes(q), q, tsh._topo()),
                 lambda: d_sgd.init(tsh._nodes(q), tsh._topo(), q)):
        with pytest.raises(ValueError, match="--device-sampling-cached .*needs --device-sampling"):
            call()
    q = _params()
    del q["algorithm"]["device-training"], q["algorithm"][tsh.SAMPLE]
    with pytest.raises(ValueError, match="--device-sampling .*--device-training"):
        train.check_eligible(tsh._nodes(q), q, tsh._topo())


def test_cli_flag_writes_its_key_and_needs_device_sampling(tmp_path, monkeypatch, capsys):
    from niidmix import d_sgd
    monkeypatch.setattr(d_sgd, "load_topology", lambda rundir: tsh._topo())
    cases = ((["--device-training", "--device-sampling", "--device-sampling-cached"], (True, True)),
             (["--device-training-sample", "--device-sampling"], (True, None)))
    for i, (argv, want) in enumerate(cases):
        run = tmp_path / f"run{i}"
        run.mkdir()
        (run / "params.json").write_text(json.dumps({"topology": {"name": "sample"}}))
        d_sgd.main(["--rundir", str(run)] + argv)
        alg = json.loads((run / "params.json").read_text())["algorithm"]
        assert (alg.get("device-sampling"), alg.get("device-sampling-cached")) == want, argv
    run = tmp_path / "alone"
    run.mkdir()
    (run / "params.json").write_text(json.dumps({"topology": {"name": "ring"}}))
    with pytest.raises(SystemExit):
        d_sgd.main(["--rundir", str(run), "--device-training", "--device-sampling-cached"])
    assert "--device-sampling-cached needs --device-sampling" in capsys.readouterr().err
    assert "algorithm" not in json.loads((run / "params.json").read_text())


def test_header_library_and_ops_declare_the_new_names():
    from niidmix import _lib, ops
    text = open(os.path.join(REPO, "include", "niidmix.h")).read()
    assert re.search(r"^int niidmix_epoch_perm_i32\(uint32_t seed,", text, re.M)
    assert re.search(r"^int niidmix_take_batches_i32\(const int32_t \*perm,", text, re.M)
    assert re.search(r"^int64_t niidmix_epoch_perm_max_len\(void\);", text, re.M)
    assert re.search(r"^int64_t niidmix_epoch_perm_scratch_bytes\(int64_t n_jobs, int64_t max_len\);", text, re.M)
    assert "#define NIIDMIX_ABI_VERSION 6" in text and _lib.lib.niidmix_abi_version() == 6 == _lib.ABI_VERSION
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("niidmix_epoch_perm_i32", "niidmix_take_batches_i32", "niidmix_epoch_perm_max_len",
                 "niidmix_epoch_perm_scratch_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    most = ops.epoch_perm_max_len()
    assert _lib.lib.niidmix_epoch_perm_max_len() == most >= 2 ** 20
    assert str(most) in text                                        # the chosen value is in the header
    # 0 up to what one workgroup sorts, else n_jobs * pow2(max_len) * 8
    for n, length, want in ((1, 1, 0), (7, 8192, 0), (1, 8193, 16384 * 8), (3, 16384, 3 * 16384 * 8),
                            (5, 16385, 5 * 32768 * 8), (2, 60000, 2 * 65536 * 8), (1, most, most * 8)):
        assert ops.epoch_perm_scratch_bytes(n, length) == want, (n, length)
    for name in ("epoch_perm", "take_batches"):
        assert hasattr(torch.ops.niidmix, name) and callable(getattr(ops, name))
    # the parent's names stay as they were
    assert ops.draw_batches_max_len() == 8192


def test_epoch_perm_argument_errors_without_gpu():
    """Validation happens before any HIP call: the documented codes come back on a CPU-only host
    (the made-up addresses are never dereferenced)."""
    from niidmix import _lib
    L = _lib.lib
    F = L.niidmix_epoch_perm_i32
    most = L.niidmix_epoch_perm_max_len()
    n, length, plen = 3, 20000, 70000
    need = L.niidmix_epoch_perm_scratch_bytes(n, length)
    assert need == n * 32768 * 8
    A = [(i + 1) << 24 for i in range(6)]           # rank, seg_len, epoch, perm_off, perm, scratch
    names = ("rank", "seg_len", "epoch", "perm_off", "perm", "scratch")

    def call(n_jobs=n, max_len=length, perm_len=plen, scratch_bytes=need, **ptr):
        a = [ptr.get(k, v) for k, v in zip(names, A)]
        return F(SEED, *a[:4], n_jobs, max_len, a[4], perm_len, a[5], scratch_bytes, None)

    for name in names:
        assert call(**{name: None}) == _lib.EINVAL and b"null" in L.niidmix_last_error(), name
    assert call(n_jobs=0) == _lib.EINVAL and call(n_jobs=-1) == _lib.EINVAL
    assert call(max_len=0) == _lib.EINVAL and call(perm_len=0) == _lib.EINVAL
    assert call(max_len=most + 1, scratch_bytes=1 << 40) == _lib.EUNSUPPORTED and b"max_len" in L.niidmix_last_error()
    assert call(n_jobs=1 << 31, scratch_bytes=1 << 60) == _lib.EUNSUPPORTED
    assert call(scratch_bytes=need - 1) == _lib.EINVAL and b"scratch" in L.niidmix_last_error()
    assert call(scratch_bytes=0) == _lib.EINVAL
    assert call(scratch=A[5] + 8) == _lib.EINVAL                     # not 16-B aligned
    for name, words in (("rank", n), ("seg_len", n), ("epoch", n), ("perm_off", 2 * n)):
        assert call(**{name: A[4] + 4 * (plen - 1)}) == _lib.EALIAS, name        # an input inside perm
        assert call(**{name: A[4] - 4 * (words - 1)}) == _lib.EALIAS, name       # its tail on perm's head
        assert call(**{name: A[5] + need - 4}) == _lib.EALIAS, name              # inside the scratch
    assert call(perm=A[5] + need - 4) == _lib.EALIAS                 # the outputs on each other
    # a short call needs no scratch: only then may it be null, and its size is not looked at
    assert call(max_len=8192, scratch=None, scratch_bytes=0, n_jobs=0) == _lib.EINVAL
    assert b"null" not in L.niidmix_last_error()
    # (no call here passes every check: that one would launch on the made-up addresses)


def test_take_batches_argument_errors_without_gpu():
    from niidmix import _lib
    L = _lib.lib
    F = L.niidmix_take_batches_i32
    most = L.niidmix_epoch_perm_max_len()
    n, b, plen = 5, 8, 1000
    A = [(i + 1) << 24 for i in range(7)]    # perm, perm_off, seg_start, seg_len, cursor, idx, len
    names = ("perm", "perm_off", "seg_start", "seg_len", "cursor", "batch_idx", "batch_len")

    def call(n_jobs=n, b_max=b, perm_len=plen, **ptr):
        a = [ptr.get(k, v) for k, v in zip(names, A)]
        return F(a[0], perm_len, *a[1:5], n_jobs, b_max, a[5], a[6], None)

    for name in names:
        assert call(**{name: None}) == _lib.EINVAL and b"null" in L.niidmix_last_error(), name
    assert call(n_jobs=0) == _lib.EINVAL and call(n_jobs=-1) == _lib.EINVAL
    assert call(b_max=0) == _lib.EINVAL and call(perm_len=0) == _lib.EINVAL
    assert call(b_max=most + 1) == _lib.EUNSUPPORTED and b"b_max" in L.niidmix_last_error()
    assert call(n_jobs=1 << 31) == _lib.EUNSUPPORTED
    for name in names[:5]:                          # an input inside either output
        assert call(**{name: A[5] + 4 * (n * b - 1)}) == _lib.EALIAS, name
        assert call(**{name: A[6] + 4 * (n - 1)}) == _lib.EALIAS, name
    assert call(perm_off=A[6] - 4 * (2 * n - 1)) == _lib.EALIAS      # int64 entries: 2 n words
    assert call(batch_len=A[5] + 4 * (n * b - 1)) == _lib.EALIAS     # the outputs on each other


def test_ops_refuse_cpu_tensors():
    from niidmix import ops
    v = lambda dt=torch.int32: torch.zeros(2, dtype=dt)              # noqa: E731
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.epoch_perm(SEED, v(), v(), v(), v(torch.int64), 4, torch.zeros(8, dtype=torch.int32),
                       torch.zeros(0, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.take_batches(torch.zeros(8, dtype=torch.int32), v(torch.int64), v(), v(), v(),
                         torch.zeros(2, 4, dtype=torch.int32), v())


def test_sampler_state_names_the_rows_to_sort():
    """Graph rounds: every row is stale in round 0 and again in the round after the one that
    reported its epoch_done, never in between; the tag is the epoch the next batch comes from."""
    from niidmix.sampling import SamplerState
    lengths, b = [10, 4, 7], 4                       # 3, 1 and 2 batches per epoch
    st = SamplerState([5, 6, 7], lengths, b, epochs=[0, 3, 0])
    assert st.cached.tolist() == [-1, -1, -1]
    rows = np.arange(3)
    began = np.ones(3, dtype=bool)                   # the coming batch is an epoch's first
    for _ in range(13):
        stale = st.stale(rows)
        assert stale.tolist() == rows[began].tolist()
        assert np.array_equal(st.stale(rows), stale)                 # asking changes nothing
        st.mark_cached(stale)
        assert st.stale(rows).size == 0 and np.array_equal(st.cached, st.epoch)
        epoch, cursor, done = st.advance(rows)
        assert np.array_equal(st.cached, epoch)      # this round's batches came from the cached epochs
        assert (cursor == 0).tolist() == began.tolist()
        began = np.array([done[r] for r in (5, 6, 7)])
    assert st.epoch.tolist() == [4, 16, 6]


def test_sampler_state_sorts_only_the_rows_a_sample_draws():
    """A sample run: rows advance at different rates; a row is stale exactly when it is drawn for
    the first time or for the first time after its epoch ended, however long ago that was; rows
    outside the sample are never named."""
    from niidmix.sampling import SamplerState
    st = SamplerState([10, 11, 12, 13], [5, 3, 8, 2], 2, epochs=[0, 7, 0, 1])
    samples = ([2, 0], [1, 3, 0], [0, 1], [3, 2], [2, 3], [0, 2], [2, 1, 0])
    fresh = {}                                       # row -> the next draw begins an epoch
    sorted_rows = []
    for rows in samples:
        stale = st.stale(rows)
        want = [r for r in rows if fresh.get(r, True)]
        assert stale.tolist() == want, rows          # in the sample's order
        sorted_rows.append(want)
        st.mark_cached(stale)
        before = st.cached.copy()
        epoch, _, done = st.advance(rows)
        assert np.array_equal(st.cached, before) and np.array_equal(st.cached[rows], epoch)
        for r, rank in zip(rows, st.rank[rows].tolist()):
            fresh[r] = done[rank]
    # worked by hand: batches per epoch are 3, 2, 4 and 1
    assert sorted_rows == [[2, 0], [1, 3], [], [3], [3], [0], [2, 1]]
    assert st.cached.tolist() == [1, 8, 1, 3] and st.epoch.tolist() == [1, 8, 1, 4]
