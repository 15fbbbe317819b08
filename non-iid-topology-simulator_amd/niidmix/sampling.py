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

`--device-sampling-torch-stream` fills the same cache with the CPU path's own permutations instead:
what one DataLoader(range(n), batch_size, shuffle=True) per node draws from the global torch RNG.
torch_permutation restates torch.randperm on the CPU (MT19937 and a Fisher-Yates loop; the oracle
of niidmix::torch_randperm), LoaderDraws the loaders' draws from the global generator.
"""
import numpy as np
import torch

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


# ------------------------------------------------------------------------------------------------
# torch's stream (--device-sampling-torch-stream)
MT_N, MT_M = 624, 397


def mt19937_words(seed, count):
    """The first `count` 32-bit outputs of MT19937 after init_genrand(seed & 0xffffffff) -- what
    ATen's CPU generator yields after manual_seed(seed): uint32 array."""
    mt = np.empty(MT_N, dtype=np.uint64)
    s = int(seed) & MASK
    mt[0] = s
    for j in range(1, MT_N):
        s = (1812433253 * (s ^ (s >> 30)) + j) & MASK
        mt[j] = s
    out = np.empty(-(-int(count) // MT_N) * MT_N, dtype=np.uint64)
    up, low, one = np.uint64(0x80000000), np.uint64(0x7FFFFFFF), np.uint64(1)
    for base in range(0, out.size, MT_N):
        # the twist in three stretches: word k + 397 (mod 624) is old for k < 227 and new after;
        # word k + 1 is old except for k = 623, whose successor is the new word 0
        for a, b in ((0, MT_N - MT_M), (MT_N - MT_M, 2 * (MT_N - MT_M)), (2 * (MT_N - MT_M), MT_N)):
            k = np.arange(a, b)
            nxt = mt[(k + 1) % MT_N]
            y = (mt[k] & up) | (nxt & low)
            mt[k] = mt[(k + MT_M) % MT_N] ^ (y >> one) ^ ((nxt & one) * np.uint64(0x9908B0DF))
        y = mt.copy()
        y ^= y >> np.uint64(11)
        y ^= (y << np.uint64(7)) & np.uint64(0x9D2C5680)
        y ^= (y << np.uint64(15)) & np.uint64(0xEFC60000)
        y ^= y >> np.uint64(18)
        out[base:base + MT_N] = y
    return out[:int(count)].astype(np.uint32)


def torch_permutation(seed, n):
    """torch.randperm(n, generator=g) on the CPU after g.manual_seed(seed), for n below 2^32 / 20
    (ATen's randperm_cpu): a = 0 .. n-1, then for i in 0 .. n-2: z = next_u32 % (n - i) and
    a[i], a[i + z] swap.  Only the seed's low 32 bits count.  int64 array."""
    n = int(n)
    a = list(range(n))
    z = mt19937_words(seed, max(n - 1, 0)).astype(np.int64) % (n - np.arange(max(n - 1, 0)))
    for i, zi in enumerate(z.tolist()):
        a[i], a[i + zi] = a[i + zi], a[i]
    return np.asarray(a, dtype=np.int64)


class LoaderDraws:
    """What the CPU path's loaders (train.index_loader, d_sgd._loader) draw from the global torch
    generator, without the loaders.  A DataLoader iterator draws one int64 random_() when it is
    created (its base seed, unused without workers) and its sampler one more at the first next():
    the seed of the epoch's randperm.  train.draw creates a node's next loader in the round its
    epoch ends, so a round draws, for each of its rows in order, "the seed if the row begins an
    epoch, then a base seed if its epoch ends".  One random_() over a tensor of that many values
    yields the values of as many scalar draws and leaves the generator in the same state."""

    @staticmethod
    def at_init(n):
        """The base seeds of the n loaders init() would create."""
        torch.empty(int(n), dtype=torch.int64).random_()

    @staticmethod
    def round(stale_mask, done_mask):
        """One round's draws for its rows in order (boolean arrays: the row begins an epoch, its
        epoch ends this round).  Returns the low 32 bits of the seeds of the rows that begin an
        epoch, in row order: int64 array of values below 2^32."""
        stale, done = np.asarray(stale_mask, dtype=bool), np.asarray(done_mask, dtype=bool)
        per_row = stale.astype(np.int64) + done
        m = int(per_row.sum())
        if m == 0:
            return np.empty(0, dtype=np.int64)
        values = torch.empty(m, dtype=torch.int64).random_().numpy()
        first = np.cumsum(per_row) - per_row             # a row's first draw is its seed
        return values[first[stale]] & MASK
