"""niidmix.batches.IndexLayout and the choice of a batch source, which need no GPU.  Every expected
number is written out here from the layout's table (indices [n, b_max], lengths [n], sample_tail
[3, n] on a sample run, a pad word to an even count and perm_off int64 [2, n] when cached, jobs
[5, n] under device sampling, sort_lists [3, n] when cached), not taken from the layout."""
import pytest
import torch

# (sample, sampling, cached): a graph round, a sample round, and both under each sampling mode
MODES = [(False, False, False), (True, False, False), (True, True, False), (True, True, True),
         (False, True, False), (False, True, True)]
# n = 3, b_max = 2: name -> (first word, one past the last), and the block's length
SPANS = {
    (False, False, False): ({"indices": (0, 6), "lengths": (6, 9)}, 9),
    (True, False, False): ({"indices": (0, 6), "lengths": (6, 9), "sample_tail": (9, 18)}, 18),
    (True, True, False): ({"indices": (0, 6), "lengths": (6, 9), "sample_tail": (9, 18), "jobs": (18, 33)},
                          33),
    # 18 words so far: even, no pad
    (True, True, True): ({"indices": (0, 6), "lengths": (6, 9), "sample_tail": (9, 18), "perm_off": (18, 30),
                          "jobs": (30, 45), "sort_lists": (45, 54)}, 54),
    (False, True, False): ({"indices": (0, 6), "lengths": (6, 9), "jobs": (9, 24)}, 24),
    # 9 words so far: word 9 is the pad
    (False, True, True): ({"indices": (0, 6), "lengths": (6, 9), "perm_off": (10, 22), "jobs": (22, 37),
                           "sort_lists": (37, 46)}, 46),
}
SHAPES = {"indices": (3, 2), "lengths": (3,), "sample_tail": (3, 3), "perm_off": (2, 3), "jobs": (5, 3),
          "sort_lists": (3, 3)}


def _layout(n, b_max, mode):
    from niidmix.batches import IndexLayout
    return IndexLayout(n, b_max, *mode)


def _first(lay, block, name):
    """The first int32 word of the view `name`, from its address."""
    return (lay.view(block, name).data_ptr() - block.data_ptr()) // 4


@pytest.mark.parametrize("mode", MODES)
def test_lists_lie_where_the_table_puts_them(mode):
    lay = _layout(3, 2, mode)
    spans, words = SPANS[mode]
    assert lay.words == words
    block = torch.zeros(words, dtype=torch.int32)
    for name, (first, last) in spans.items():
        v = lay.view(block, name)
        assert tuple(v.shape) == SHAPES[name], name
        assert v.dtype == (torch.int64 if name == "perm_off" else torch.int32), name
        assert _first(lay, block, name) == first, name
        assert v.numel() * v.element_size() == (last - first) * 4, name
    for name in set(SHAPES) - set(spans):                   # a list the mode does not have
        with pytest.raises(KeyError):
            lay.view(block, name)


def test_pad_word_appears_at_an_odd_count():
    lay = _layout(3, 1, (True, True, True))                 # 3 + 12 = 15 words before perm_off
    block = torch.zeros(lay.words, dtype=torch.int32)
    assert _first(lay, block, "sample_tail") == 6 and _first(lay, block, "perm_off") == 16
    assert _first(lay, block, "jobs") == 28 and _first(lay, block, "sort_lists") == 43
    assert lay.words == 52


def test_no_pad_word_at_an_even_count():
    lay = _layout(2, 3, (False, True, True))                # 6 + 2 = 8 words before perm_off
    block = torch.zeros(lay.words, dtype=torch.int32)
    assert _first(lay, block, "perm_off") == 8 and _first(lay, block, "jobs") == 16
    assert _first(lay, block, "sort_lists") == 26 and lay.words == 32


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,b_max", [(1, 1), (2, 3), (3, 1), (3, 2), (5, 7), (16, 25), (1000, 125)])
def test_words(mode, n, b_max):
    sample, sampling, cached = mode
    words = n * b_max + (4 if sample else 1) * n
    if cached:
        words += words % 2
        words += 4 * n
    if sampling:
        words += (8 if cached else 5) * n
    assert _layout(n, b_max, mode).words == words


@pytest.mark.parametrize("n,b_max,sample", [(3, 2, True), (3, 2, False), (3, 1, True), (2, 3, False),
                                            (5, 7, True)])
def test_perm_off_is_int64_on_eight_bytes(n, b_max, sample):
    lay = _layout(n, b_max, (sample, True, True))
    block = torch.zeros(lay.words, dtype=torch.int32)
    v = lay.view(block, "perm_off")
    assert v.dtype == torch.int64 and tuple(v.shape) == (2, n)
    assert (v.data_ptr() - block.data_ptr()) % 8 == 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,b_max", [(3, 2), (3, 1), (2, 3), (5, 7)])
def test_views_cover_the_block_without_overlap(mode, n, b_max):
    lay = _layout(n, b_max, mode)
    block = torch.full((lay.words,), -1, dtype=torch.int32)
    sample, sampling, cached = mode
    names = ["indices", "lengths"] + ["sample_tail"] * sample + ["perm_off"] * cached + \
        ["jobs"] * sampling + ["sort_lists"] * cached
    size = {"indices": n * b_max, "lengths": n, "sample_tail": 3 * n, "perm_off": 4 * n, "jobs": 5 * n,
            "sort_lists": 3 * n}
    for tag, name in enumerate(names, start=1):
        # an int64 element is two words: the tag in both
        lay.view(block, name).fill_(tag | tag << 32 if name == "perm_off" else tag)
    for tag, name in enumerate(names, start=1):             # a later view wrote over none of an earlier one
        assert int((block == tag).sum()) == size[name], name
    pad = int(cached and (n * b_max + (4 if sample else 1) * n) % 2 == 1)
    assert int((block == -1).sum()) == pad
    if pad:
        assert int(block[n * b_max + (4 if sample else 1) * n]) == -1


def test_copy_ranges():
    nb, n = 6, 3                                             # n = 3, b_max = 2
    # graph rounds under --device-sampling-cached: word 9 is the pad
    off0, job0, words = 10, 22, 46
    lay = _layout(3, 2, (False, True, True))
    assert lay.copy_range(False) == (job0 + 3 * n, job0 + 5 * n) == (31, 37)      # jobs[3:5]
    assert lay.copy_range(True) == (off0 + 2 * n, words) == (16, 46)
    # sample rounds under it
    job0, words = 30, 54
    lay = _layout(3, 2, (True, True, True))
    assert lay.copy_range(False) == (nb + n, job0 + 5 * n) == (9, 45)
    assert lay.copy_range(True) == (nb + n, words) == (9, 54)
    # plain --device-sampling never sorts
    assert _layout(3, 2, (False, True, False)).copy_range(False) == (9 + 3 * n, 9 + 5 * n) == (18, 24)
    assert _layout(3, 2, (True, True, False)).copy_range(False) == (nb + n, 18 + 5 * n) == (9, 33)
    # without --device-sampling the whole block
    assert _layout(3, 2, (False, False, False)).copy_range(False) == (0, 9)
    assert _layout(3, 2, (True, False, False)).copy_range(False) == (0, 18)


@pytest.mark.parametrize("sample", [False, True])
def test_batch_source_of_a_mode(sample):
    from niidmix import batches
    assert batches.source_class(sample, False, False) is batches.LoaderSource
    assert batches.source_class(sample, True, False) is batches.DeviceSource
    assert batches.source_class(sample, True, True) is batches.CachedSource
    assert issubclass(batches.CachedSource, batches.DeviceSource)
    assert not issubclass(batches.DeviceSource, batches.LoaderSource)
