"""The sample stream of `--device-sampling`, restated on the host in numpy.

Under the flag a node's batches do not come from torch's DataLoader (and the global torch RNG) but
from a stream of the project's own, defined in integers only so that the device kernel
(niidmix::draw_batches, csrc/sampling.inc) and this module agree exactly:

    key          sample position i (0 <= i < len) of the node of rank r in epoch e, run seed s
                 (params['meta']['seed']), gets the 32-bit key
                     k_i = word (i & 3) of Philox4x32-10(counter (i >> 2, e, 0, 0),
                                                        key (s & 0xffffffff, r))
    permutation  epoch e visits the positions in ascending order of the 64-bit composites
                 (k_i << 32) | i  (distinct by construction: no ties)
    batching     consecutive slices of B = batch-size positions, the last one short, as
                 DataLoader(shuffle=True, drop_last=False); the batch that reaches the end of the
                 permutation reports epoch_done, increments the epoch and resets the cursor

This module is the tests' oracle for the kernel, and SamplerState tells the host every round's
epoch_done flags and batch lengths without a copy back from the device.  Under
`--device-sampling-cached` the same permutations are sorted once per epoch into a device cache
(niidmix::epoch_perm, sliced by niidmix::take_batches); SamplerState then also records which
epoch's permutation each row's part of the cache holds.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57           # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85           # Weyl increments of the key
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11; Random123).  `counter`: four arrays (or ints) of
    32-bit words, broadcast against each other; `key`: two.  Returns four uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & MASK for c in counter])
    k0, k1 = (np.asarray(k, dtype=np.uint64) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                    # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def keys(seed, rank, epoch, length):
    """The 32-bit keys k_0 .. k_{length-1} of one node and epoch."""
    n4 = (int(length) + 3) // 4
    words = philox4x32_10((np.arange(n4), int(epoch), 0, 0), (int(seed) & MASK, int(rank) & MASK))
    return np.stack(words, axis=1).reshape(-1)[:int(length)]


def epoch_permutation(seed, rank, epoch, length):
    """Epoch `epoch`'s permutation of 0 .. length-1 for the node of rank `rank`: int64 array."""
    k = keys(seed, rank, epoch, length).astype(np.uint64)
    comp = (k << np.uint64(32)) | np.arange(int(length), dtype=np.uint64)
    return (np.sort(comp) & np.uint64(MASK)).astype(np.int64)


def batch(seed, rank, epoch, cursor, length, b):
    """The batch that starts at position `cursor` of the epoch's permutation: at most b
    segment-local sample positions (int64), fewer at the end of the epoch."""
    if not 0 <= cursor < length or b < 1:
        raise ValueError(f"cursor {cursor} outside 0..{length - 1}, or batch size {b} < 1")
    return epoch_permutation(seed, rank, epoch, length)[cursor:cursor + b]


class SamplerState:
    """Epoch and cursor of every node of a list, on the host: numpy arrays `epoch`, `cursor`,
    `length` (and `rank`), one entry per row of the list; `cached` is the epoch whose permutation
    the device cache of --device-sampling-cached holds for the row (-1: none)."""

    def __init__(self, ranks, lengths, b, epochs=None):
        self.rank = np.asarray(ranks, dtype=np.int64)
        self.length = np.asarray(lengths, dtype=np.int64)
        self.b = int(b)
        if self.b < 1 or self.length.shape != self.rank.shape or (self.length < 1).any():
            raise ValueError("SamplerState: batch size and every length must be >= 1")
        self.epoch = np.zeros_like(self.length) if epochs is None else np.asarray(epochs, dtype=np.int64).copy()
        self.cursor = np.zeros_like(self.length)
        # --device-sampling-cached: the epoch whose permutation the device cache holds, -1 for none
        self.cached = np.full_like(self.length, -1)

    def stale(self, rows):
        """Those of the rows `rows` (distinct, any order; their order is kept) whose cached
        permutation is not the one their NEXT batch comes from: they are sorted before it is drawn."""
        rows = np.asarray(rows, dtype=np.int64)
        return rows[self.cached[rows] != self.epoch[rows]]

    def mark_cached(self, rows):
        """The cache now holds the current epoch's permutation of the rows `rows`."""
        rows = np.asarray(rows, dtype=np.int64)
        self.cached[rows] = self.epoch[rows]

    def advance(self, rows):
        """One batch of each of the rows `rows` (distinct, any order): returns (epoch, cursor,
        {rank: epoch_done}) -- the rows' epoch and cursor of THIS round's batch (int64 arrays in
        the order of `rows`; the batch holds min(b, length - cursor) samples) -- and moves their
        state past it.  Other rows are not touched."""
        rows = np.asarray(rows, dtype=np.int64)
        epoch, cursor = self.epoch[rows], self.cursor[rows]
        done = cursor + self.b >= self.length[rows]
        self.epoch[rows] = epoch + done
        self.cursor[rows] = np.where(done, 0, cursor + self.b)
        return epoch, cursor, dict(zip(self.rank[rows].tolist(), done.tolist()))
