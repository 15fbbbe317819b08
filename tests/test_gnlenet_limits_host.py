"""tests/test_gpu_gnlenet_limits.py without a GPU: every seeded case's float64 ambiguity
(evaluation) and separation (gradient) from the CPU references alone, so that a bad seed is caught
here; the tile rule, the activation-slot threshold and the M-tile coverage that file relies on."""
import pytest

import test_gpu_gnlenet_limits as tl


@pytest.mark.parametrize("i", range(len(tl.EVAL)), ids=tl._eval_ids)
def test_evaluation_cases_are_unambiguous(i):
    d, jobs = tl.limit_case(i)
    e32, ambiguous, pairs = tl.yardstick(d, jobs)
    assert e32 > 0 and ambiguous <= 0.01 * pairs, "the case is ambiguous in float64: reseed it"


@pytest.mark.parametrize("op,slots", [(tl.PLAIN, True), (tl.PLAIN, False), (tl.MFMA, False)])
def test_loop_patterns_are_unambiguous(op, slots):
    d, pats = tl.loop_case(op, tl.slot_shape() if slots else tl.LOOP_SHAPE)
    tile = tl.tile_of(op, d["shape"])
    assert len(set(pats)) == len(pats) == 7 and all(1 <= n <= tile and s + n <= tl.M for _, s, n in pats)
    e32, ambiguous, pairs = tl.yardstick(d, pats)
    assert e32 > 0 and ambiguous <= 0.01 * pairs, "the case is ambiguous in float64: reseed it"


@pytest.mark.parametrize("name", ["big", "wide", "long", "zero"])
def test_gradient_cases_are_separated(name):
    d = tl.grad_case(name)
    assert d["lens"] == {"big": [2, 1], "wide": [2], "long": [9, 6, 1], "zero": [3, 0, 2]}[name]
    tl.assert_separated(d)


def test_big_case_takes_its_samples_from_each_rows_half_of_the_pool():
    p = tl.BIG_POOL
    assert [len(row) for row in tl.BIG_PICK] == [2, 1]
    assert all(r * p <= i < (r + 1) * p for r, row in enumerate(tl.BIG_PICK) for i in row)
    assert len({i for row in tl.BIG_PICK for i in row}) == 3


def test_tile_rule_facts():
    """The tile table the GPU file derives its M-tile counts from, through the library's size
    function (12 B per (job, tile), 0 where the kernel refuses the shape) and ops.gn_mfma_tile."""
    from niidmix import _lib, ops
    size = _lib.lib.niidmix_gnlenet_eval_rows_mfma_scratch_bytes
    facts = dict(tl.MFMA_TILE)
    facts[tl.MFMA_REFUSED[1:3]] = 0
    assert facts[(42, 42)] == facts[(64, 15)] == 2 and facts[(44, 15)] == facts[(28, 28)] == 4
    for hw, tile in facts.items():
        assert ops.gn_mfma_tile(*hw) == tile, hw
        assert size(1, 8, 1, *hw, 10) == ((-(-8 // tile) * 12 + 15) // 16 * 16 if tile else 0), hw


def test_activation_slots_begin_at_the_slot_shape():
    from niidmix._lib import lib
    size = lib.niidmix_gnlenet_eval_rows_scratch_bytes
    cin, h, w, c = tl.slot_shape()
    assert h == w and size(1, 1, cin, h, w, c) > 16
    assert size(1, 1, cin, h - 1, w - 1, c) == 16
    # a slot per workgroup up to the cap: the same bytes of slots at 4096 and at 4096 + 300 jobs
    slots = lambda n: size(n, 2, cin, h, w, c) - (n * 12 + 15) // 16 * 16  # noqa: E731
    assert slots(tl.SLOT_CAP + 300) == slots(tl.SLOT_CAP) == tl.SLOT_CAP * slots(1)


def test_mtile_counts_under_test_cover_every_instantiation():
    tl.check_mtile_coverage()
