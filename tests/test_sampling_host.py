"""--device-sampling, the parts that need no GPU: the sample stream's host restatement
(niidmix.sampling: Philox4x32-10, the epoch permutation, the batches), the SamplerState bookkeeping
against train.draw with real index loaders, the flag and its refusals, and the C entry point's
declaration and argument checks."""
import ctypes
import itertools
import json
import os
import re
from collections import Counter

import numpy as np
import pytest
import torch

import test_train_sample_host as tsh
from conftest import REPO

SEED = 2027
LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 1000)


def test_philox_known_answers():
    """Random123's published vectors for Philox4x32-10 (kat_vectors): zero counter and key, all
    ones, and the digits of pi."""
    from niidmix.sampling import philox4x32_10

    def words(counter, key):
        return [int(w) for w in philox4x32_10(counter, key)]
    assert words((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = 0xffffffff
    assert words((f, f, f, f), (f, f)) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert words((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    # vectorised over the counter: the same words as one call each
    got = philox4x32_10((np.arange(5), 7, 0, 0), (SEED, 3))
    for q in range(5):
        assert [int(w[q]) for w in got] == words((q, 7, 0, 0), (SEED, 3))


def test_keys_follow_the_contract():
    """k_i is word (i & 3) of the call with counter (i >> 2, epoch, 0, 0) and key (seed, rank); the
    permutation is the order of (k_i << 32) | i."""
    from niidmix import sampling
    keys = sampling.keys(SEED, 5, 9, 11)
    for i in range(11):
        assert int(keys[i]) == int(sampling.philox4x32_10((i >> 2, 9, 0, 0), (SEED, 5))[i & 3])
    comp = sorted((int(k) << 32) | i for i, k in enumerate(keys))
    assert sampling.epoch_permutation(SEED, 5, 9, 11).tolist() == [c & 0xffffffff for c in comp]
    # only the seed's low 32 bits count
    assert np.array_equal(sampling.keys(SEED + (1 << 32), 5, 9, 11), keys)


@pytest.mark.parametrize("length", LENGTHS)
def test_epoch_permutation_is_a_permutation(length):
    from niidmix.sampling import batch, epoch_permutation
    p = epoch_permutation(SEED, 3, 0, length)
    assert p.dtype == np.int64 and sorted(p.tolist()) == list(range(length))
    assert np.array_equal(p, epoch_permutation(SEED, 3, 0, length))            # repeated call
    if length >= 5:                         # shorter ones may coincide by chance
        assert not np.array_equal(p, epoch_permutation(SEED, 3, 1, length))    # another epoch
        assert not np.array_equal(p, epoch_permutation(SEED, 4, 0, length))    # another rank
        assert not np.array_equal(p, epoch_permutation(SEED + 1, 3, 0, length))
    # batches are consecutive slices, the last one short
    b = 4
    got = [batch(SEED, 3, 0, c, length, b) for c in range(0, length, b)]
    assert np.array_equal(np.concatenate(got), p) and all(len(g) == b for g in got[:-1])
    with pytest.raises(ValueError):
        batch(SEED, 3, 0, length, length, b)


def test_permutations_of_three_are_uniform():
    """6000 epochs of one rank, length 3: each of the 6 orders 1000 times within 5 sigma
    (sigma = sqrt(6000 * 1/6 * 5/6) = 28.9).  Deterministic given the seed."""
    from niidmix.sampling import epoch_permutation
    count = Counter(tuple(epoch_permutation(SEED, 0, e, 3).tolist()) for e in range(6000))
    assert sorted(count) == sorted(itertools.permutations(range(3)))
    assert all(850 <= v <= 1150 for v in count.values()), count


@pytest.mark.parametrize("length,b", [(60, 125), (125, 125), (126, 125), (600, 128), (7, 1), (1, 4)])
def test_sampler_state_counts_as_train_draw_does(length, b):
    """Three epochs: batch lengths, epoch_done flags and node['epoch'] equal those of train.draw
    with real index loaders on a train-set of the same length (sizes and flags, not contents)."""
    from niidmix import train
    from niidmix.sampling import SamplerState
    params = {"algorithm": {"batch-size": b}}
    node = {"rank": 4, "epoch": 0, "train-set": list(range(length))}
    node["train-iterator"] = train.index_loader(node, params)
    st = SamplerState([4], [length], b)
    want, got = [], []
    while node["epoch"] < 3:
        batches, done = train.draw([node], params)
        want.append((batches[0].numel(), done, node["epoch"]))
        epoch, cursor, flags = st.advance([0])
        got.append((min(b, length - int(cursor[0])), flags, int(st.epoch[0])))
        assert int(epoch[0]) == want[-1][2] - int(done[4])          # the epoch the batch came from
    assert got == want and len(got) == 3 * -(-length // b)
    assert int(st.cursor[0]) == 0 and int(st.epoch[0]) == 3


def test_sampler_state_advances_the_listed_rows_only():
    from niidmix.sampling import SamplerState
    st = SamplerState([10, 11, 12, 13], [5, 3, 8, 2], 2, epochs=[0, 7, 0, 1])
    e, c, done = st.advance([2, 0])                                  # the sample's order
    assert e.tolist() == [0, 0] and c.tolist() == [0, 0] and done == {12: False, 10: False}
    assert st.cursor.tolist() == [2, 0, 2, 0] and st.epoch.tolist() == [0, 7, 0, 1]
    e, c, done = st.advance([1, 3, 0])
    assert e.tolist() == [7, 1, 0] and c.tolist() == [0, 0, 2]
    assert done == {11: False, 13: True, 10: False}
    assert st.cursor.tolist() == [4, 2, 2, 0] and st.epoch.tolist() == [0, 7, 0, 2]
    e, c, done = st.advance([0, 1])
    assert c.tolist() == [4, 2] and done == {10: True, 11: True}
    assert st.cursor.tolist() == [0, 0, 2, 0] and st.epoch.tolist() == [1, 8, 0, 2]
    with pytest.raises(ValueError):
        SamplerState([0], [0], 2)


def _params(**alg):
    p = tsh._params(**{"device-sampling": True, **alg})
    p["meta"]["seed"] = SEED
    return p


def test_flag_is_refused_without_a_training_flag_and_beyond_the_kernels_limits():
    from niidmix import d_sgd, ops, train
    most = ops.draw_batches_max_len()
    assert most >= 8192
    p = _params()
    assert train.sampling_enabled(p) and train.check_eligible(tsh._nodes(p), p, tsh._topo()) == (6, 3)
    # no training flag at all
    q = _params()
    del q["algorithm"]["device-training"], q["algorithm"][tsh.SAMPLE]
    for call in (lambda: train.check_eligible(tsh._nodes(q), q, tsh._topo()),
                 lambda: d_sgd.init(tsh._nodes(q), tsh._topo(), q)):
        with pytest.raises(ValueError, match="--device-sampling .*--device-training"):
            call()
    # a train-set over the maximum length (a range stands in for the samples: only len() is read)
    nodes = tsh._nodes(p)
    nodes[3]["train-set"] = range(most + 1)
    with pytest.raises(ValueError, match=rf"--device-sampling: node 3's train-set has {most + 1} samples"):
        train.check_eligible(nodes, p, tsh._topo())
    nodes[3]["train-set"] = nodes[2]["train-set"]
    assert train.check_eligible(nodes, p, tsh._topo()) == (6, 3)
    # a batch size over it
    q = _params(**{"batch-size": most + 1})
    with pytest.raises(ValueError, match=rf"--device-sampling: batch size {most + 1}"):
        train.check_eligible(tsh._nodes(q), q, tsh._topo())
    # the stream is keyed by the run's seed
    q = _params()
    del q["meta"]["seed"]
    with pytest.raises(ValueError, match="--device-sampling .*seed"):
        train.check_eligible(tsh._nodes(q), q, tsh._topo())


def test_init_builds_no_loaders_and_leaves_the_rng_alone():
    from niidmix import d_sgd
    p = _params()
    torch.manual_seed(5)
    before = torch.get_rng_state()
    nodes = tsh._nodes(p)
    after_nodes = torch.get_rng_state()                  # the models' initialisation
    state, step, done = d_sgd.init(nodes, tsh._topo(), p)
    assert all(n["train-iterator"] is None for n in state["nodes"])
    assert torch.equal(torch.get_rng_state(), after_nodes) and not torch.equal(before, after_nodes)
    # with the flag off: the index loaders of before
    q = tsh._params()
    state, _, _ = d_sgd.init(tsh._nodes(q), tsh._topo(), q)
    assert all(n["train-iterator"] is not None for n in state["nodes"])


def test_cli_flag_writes_its_key_and_needs_a_training_flag(tmp_path, monkeypatch, capsys):
    from niidmix import d_sgd
    monkeypatch.setattr(d_sgd, "load_topology", lambda rundir: tsh._topo())
    cases = ((["--device-training", "--device-sampling"], (True, None, None, True)),
             (["--device-training-sample", "--device-sampling"], (True, True, None, True)),
             (["--device-training-gn-lenet", "--device-sampling", "--clique-gradient"], (True, None, True, True)),
             (["--device-training"], (True, None, None, None)))
    for i, (argv, want) in enumerate(cases):
        run = tmp_path / f"run{i}"
        run.mkdir()
        (run / "params.json").write_text(json.dumps({"topology": {"name": "sample"}}))
        if "--clique-gradient" in argv:
            monkeypatch.setattr(d_sgd, "load_topology", lambda rundir: {"edges": {}, "cliques": []})
        d_sgd.main(["--rundir", str(run)] + argv)
        alg = json.loads((run / "params.json").read_text())["algorithm"]
        assert (alg.get("device-training"), alg.get(tsh.SAMPLE), alg.get(tsh.GN),
                alg.get("device-sampling")) == want, argv
    run = tmp_path / "alone"
    run.mkdir()
    (run / "params.json").write_text(json.dumps({"topology": {"name": "ring"}}))
    with pytest.raises(SystemExit):
        d_sgd.main(["--rundir", str(run), "--device-sampling"])
    assert "--device-sampling needs one of" in capsys.readouterr().err
    assert "algorithm" not in json.loads((run / "params.json").read_text())


def test_header_library_and_op_declare_the_entry_point():
    from niidmix import _lib, ops
    text = open(os.path.join(REPO, "include", "niidmix.h")).read()
    assert re.search(r"^int niidmix_draw_batches_i32\(uint32_t seed,", text, re.M)
    assert re.search(r"^int64_t niidmix_draw_batches_max_len\(void\);", text, re.M)
    assert "#define NIIDMIX_ABI_VERSION 6" in text and _lib.lib.niidmix_abi_version() == 6 == _lib.ABI_VERSION
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("niidmix_draw_batches_i32", "niidmix_draw_batches_max_len"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.lib.niidmix_draw_batches_max_len() == ops.draw_batches_max_len() >= 8192
    assert hasattr(torch.ops.niidmix, "draw_batches") and callable(ops.draw_batches)


def test_draw_batches_argument_errors_without_gpu():
    """Validation happens before any HIP call, so the documented codes come back on a CPU-only
    host too (the made-up addresses are never dereferenced)."""
    from niidmix import _lib
    L = _lib.lib
    F = L.niidmix_draw_batches_i32
    most = L.niidmix_draw_batches_max_len()
    n, b = 5, 8
    A = [(i + 1) << 20 for i in range(7)]           # rank, seg_start, seg_len, epoch, cursor, idx, len
    names = ("rank", "seg_start", "seg_len", "epoch", "cursor", "batch_idx", "batch_len")

    def call(n_jobs=n, b_max=b, **ptr):
        a = [ptr.get(k, v) for k, v in zip(names, A)]
        return F(SEED, *a[:5], n_jobs, b_max, a[5], a[6], None)

    for name in names:
        assert call(**{name: None}) == _lib.EINVAL and b"null" in L.niidmix_last_error(), name
    assert call(n_jobs=0) == _lib.EINVAL and call(n_jobs=-1) == _lib.EINVAL
    assert call(b_max=0) == _lib.EINVAL
    assert call(b_max=most + 1) == _lib.EUNSUPPORTED and b"b_max" in L.niidmix_last_error()
    assert call(n_jobs=1 << 31) == _lib.EUNSUPPORTED
    for name in names[:5]:                          # an input inside either output
        assert call(**{name: A[5] + 4 * (n * b - 1)}) == _lib.EALIAS, name
        assert call(**{name: A[6] + 4 * (n - 1)}) == _lib.EALIAS, name
    assert call(batch_len=A[5] + 4 * (n * b - 1)) == _lib.EALIAS     # the outputs on each other
    # (no call here passes every check: that one would launch on the made-up addresses)


def test_op_refuses_cpu_tensors():
    from niidmix import ops
    v = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.draw_batches(SEED, v, v.clone(), v.clone(), v.clone(), v.clone(),
                         torch.zeros(2, 4, dtype=torch.int32), v.clone())
