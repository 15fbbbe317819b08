"""How a device-training round's batches reach the device: the index block's layout and one batch
source per sampling mode (niidmix.train.DeviceTrainer builds both once).

A round's host -> device traffic is one pinned int32 block (DeviceTrainer.idx_host / idx_dev).
IndexLayout names its lists and the word range a round copies; nothing else does arithmetic on the
block.  A batch source fills the block for one round: fill(active nodes, slab rows or None, params)
returns {rank: epoch_done} once the round's indices and lengths are where the gradient op reads
them and the round's single H2D copy has been issued.  Whatever else the round sends (a sample
round's tail) is in the pinned block before fill() is called.
"""
import numpy as np
import torch

from . import ops, train


class IndexLayout:
    """The index block of a trainer of n rows and batches of up to b_max samples, in this order:

        indices      int32 [n, b_max]   always     sample indices, job j's in row j
        lengths      int32 [n]          always     batch lengths
        sample_tail  int32 [3, n]       sample     active rows, `first` flags, rows ordered
                                                   first-then-not-first
        (pad)        one int32 word     cached     when the count so far is odd: the int64 lists
                                                   start on 8 bytes
        perm_off     int64 [2, n]       cached     perm_off of the round's jobs, of the rows to sort
        jobs         int32 [5, n]       sampling   rank, seg_start, seg_len, epoch, cursor
        sort_lists   int32 [3, n]       cached     rank, seg_len, epoch of the rows to sort

    Plain arithmetic: it needs no device."""

    def __init__(self, n, b_max, sample, sampling, cached):
        self.n, self.sample, self.sampling = n, sample, sampling
        self.spans, self.words = {}, 0    # name -> (first word, one past the last, rows or None)
        for name, rows, cols, present in (("indices", n, b_max, True), ("lengths", None, n, True),
                                          ("sample_tail", 3, n, sample), ("perm_off", 2, 2 * n, cached),
                                          ("jobs", 5, n, sampling), ("sort_lists", 3, n, cached)):
            if present:
                first = self.words + (self.words & 1 if name == "perm_off" else 0)
                self.words = first + (rows or 1) * cols
                self.spans[name] = (first, self.words, rows)

    def view(self, block, name):
        """The list `name` of the int32 block `block` (pinned host, device or plain CPU tensor)."""
        first, last, rows = self.spans[name]
        v = block[first:last].view(torch.int64 if name == "perm_off" else torch.int32)
        return v if rows is None else v.view(rows, -1)

    def copy_range(self, sorting):
        """(first, last) words of a round's one H2D copy.  Without --device-sampling the whole
        block.  With it, a graph round sends its jobs' epochs and cursors (rank, seg_start and
        seg_len went up once: job j is row j), a sample round everything from its tail to the end
        of the jobs; when rows are to be sorted (`sorting`) the copy runs to the end of the block
        and a graph round's starts at the second perm_off list."""
        if not self.sampling:
            return 0, self.words
        jobs = self.spans["jobs"]
        first = self.spans["sample_tail"][0] if self.sample else \
            self.spans["perm_off"][0] + 2 * self.n if sorting else jobs[0] + 3 * self.n
        return first, self.words if sorting else jobs[1]


class LoaderSource:
    """Without --device-sampling, the CPU path's RNG stream: train.draw on the nodes' index loaders,
    the batches packed into the pinned block, the whole block in one copy."""

    def __init__(self, tr, nodes):
        self.tr = tr

    def fill(self, active, rows, params):
        """Job j = the j-th active node: its sample indices offset by its own data offset, and the
        length."""
        tr = self.tr
        batches, epoch_done = train.draw(active, params)
        bi, bl = (tr.layout.view(tr.idx_host, name).numpy() for name in ("indices", "lengths"))
        for j, (i, idx) in enumerate(zip(range(tr.n) if rows is None else rows, batches)):
            k = idx.numel()
            if k < 1 or k > tr.b_max or int(idx.max()) >= tr.offsets[i + 1] - tr.offsets[i]:
                raise ValueError(f"{tr.flag}: node {active[j]['rank']} drew a batch its train-set or "
                                 "the batch size does not allow")
            bi[j, :k] = idx.numpy() + tr.offsets[i]
            bl[j] = k
        tr.idx_dev.copy_(tr.idx_host, non_blocking=True)
        return epoch_done


class DeviceSource:
    """--device-sampling: niidmix.sampling's stream, drawn where it is consumed.  The host keeps
    (epoch, cursor) of every row (SamplerState), sends them in the one copy, and
    niidmix::draw_batches writes the indices and lengths into the block."""

    keyed = True      # the stream is keyed by params['meta']['seed']

    def __init__(self, tr, nodes):
        from .sampling import SamplerState
        self.tr = tr
        self.seed = int(tr.params["meta"]["seed"]) & 0xFFFFFFFF if self.keyed else None
        off = np.asarray(tr.offsets, dtype=np.int64)
        self.seg_start = off[:-1]
        self.sampler = SamplerState([nd["rank"] for nd in nodes], off[1:] - off[:-1], tr.b_max,
                                    epochs=[nd.get("epoch", 0) for nd in nodes])
        self.all_rows = np.arange(tr.n)
        self.host = {name: tr.layout.view(tr.idx_host, name).numpy() for name in tr.layout.spans}
        self._job_rows(self.all_rows)    # a graph round's job j is row j: these go up here, once
        tr.idx_dev.copy_(tr.idx_host)

    def _job_rows(self, rows):
        """rank, seg_start and seg_len of the jobs, which are the slab rows `rows`."""
        job, st, k = self.host["jobs"], self.sampler, len(rows)
        job[0, :k], job[1, :k], job[2, :k] = st.rank[rows], self.seg_start[rows], st.length[rows]

    def _stale(self, rows):
        """Before the rows advance: (the rows to sort first, how many of them are short)."""
        return (), 0

    def _draw(self, k, jd, stale, n_short):
        ops.draw_batches(self.seed, jd[0], jd[1], jd[2], jd[3], jd[4],
                         self.tr.dev["indices"][:k], self.tr.dev["lengths"][:k])

    def fill(self, active, rows, params):
        """`rows`: the slab rows of a sample round's active nodes, in the sample's order (only they
        advance; their rank, seg_start and seg_len go up too); None: every row.  node['epoch']
        counts as it does in train.draw."""
        tr = self.tr
        sel = self.all_rows if rows is None else rows
        k = len(sel)
        stale, n_short = self._stale(sel)
        epoch, cursor, done = self.sampler.advance(sel)
        if int(epoch.max()) >= 2 ** 31 - 1:
            raise ValueError(f"{train.FLAG_SAMPLING}: an epoch count outside int32")
        if rows is not None:
            self._job_rows(rows)
        self.host["jobs"][3, :k], self.host["jobs"][4, :k] = epoch, cursor
        for nd in active:
            nd["epoch"] += int(done[nd["rank"]])
        first, last = tr.layout.copy_range(len(stale) > 0)
        tr.idx_dev[first:last].copy_(tr.idx_host[first:last], non_blocking=True)
        self._draw(k, tr.dev["jobs"][:, :k], stale, n_short)
        return done


class CachedSource(DeviceSource):
    """--device-sampling-cached: the same stream, every epoch sorted once.  An int32 cache of
    offsets[-1] entries holds a node's permutation at its data offset; before a round's draw the
    rows whose cache is not their current epoch's are sorted by niidmix::epoch_perm, and
    niidmix::take_batches slices the cache into the block.  Their lists travel in the one copy."""

    def __init__(self, tr, nodes):
        super().__init__(tr, nodes)
        self.perm = torch.empty(tr.offsets[-1], dtype=torch.int32, device=tr.device)
        self.no_scratch = torch.empty(0, dtype=torch.int64, device=tr.device)
        self.short_max = ops.draw_batches_max_len()
        self.last_perm_jobs = self.last_perm_calls = 0      # of the last round (tests)

    def _job_rows(self, rows):
        super()._job_rows(rows)
        self.host["perm_off"][0, :len(rows)] = self.seg_start[rows]

    def _stale(self, rows):
        """The rows whose cached permutation is not their current epoch's go into the sort lists of
        the pinned block, rows of up to short_max samples first, and are marked cached."""
        st = self.sampler
        stale = st.stale(rows)
        keys = self._keys(rows, stale)
        if stale.size == 0:
            return stale, 0
        short = st.length[stale] <= self.short_max
        order = np.argsort(~short, kind="stable")
        stale, keys = stale[order], keys[order]
        m, lists = stale.size, self.host["sort_lists"]
        lists[0, :m], lists[1, :m], lists[2, :m] = st.rank[stale], st.length[stale], keys
        self.host["perm_off"][1, :m] = self.seg_start[stale]
        st.mark_cached(stale)
        return stale, int(short.sum())

    def _keys(self, rows, stale):
        """What the third sort list holds for the rows `stale` of the round's rows: their epochs."""
        return self.sampler.epoch[stale]

    def _draw(self, k, jd, stale, n_short):
        """The permutations of the rows `stale` (their lists are on the device) into the cache, then
        niidmix::take_batches."""
        self.last_perm_jobs, self.last_perm_calls = len(stale), 0
        self._sort(stale, n_short)
        ops.take_batches(self.perm, self.tr.dev["perm_off"][0, :k], jd[1], jd[2], jd[4],
                         self.tr.dev["indices"][:k], self.tr.dev["lengths"][:k])

    def _sort(self, stale, n_short):
        """niidmix::epoch_perm: the short rows in one call without scratch, the long ones in calls
        of as many rows as keep the scratch within the trainer's budget (train.cut_rows)."""
        m, length = len(stale), self.sampler.length
        lists, off = self.tr.dev["sort_lists"], self.tr.dev["perm_off"][1]

        def call(a, b, scratch):
            ops.epoch_perm(self.seed, lists[0, a:b], lists[1, a:b], lists[2, a:b], off[a:b],
                           int(length[stale[a:b]].max()), self.perm, scratch)
            self.last_perm_calls += 1
        if n_short:
            call(0, n_short, self.no_scratch)
        if m > n_short:
            longest = int(length[stale[n_short:]].max())
            budget = self.tr._budget()
            cut = train.cut_rows(m - n_short, lambda k: ops.epoch_perm_scratch_bytes(k, longest), budget)
            if cut is None:
                raise RuntimeError(f"{train.FLAG_CACHED}: {ops.epoch_perm_scratch_bytes(1, longest) / 2**30:.2f}"
                                   f" GiB of scratch to sort one row of {longest} samples exceed the "
                                   f"budget of {budget / 2**30:.2f} GiB")
            for a in range(n_short, m, cut):
                b = min(m, a + cut)
                nbytes = ops.epoch_perm_scratch_bytes(b - a, int(length[stale[a:b]].max()))
                call(a, b, torch.empty(nbytes // 8, dtype=torch.int64, device=self.tr.device))


class TorchStreamSource(CachedSource):
    """--device-sampling-torch-stream: the cache holds the CPU path's own permutations.  The host
    draws what the nodes' DataLoaders would draw from the global torch generator
    (sampling.LoaderDraws: a few int64 values a round, no loop over nodes); a row that begins an
    epoch sends the low 32 bits of its permutation's seed (as an int32 bit pattern) where
    CachedSource sends its epoch, and niidmix::torch_randperm shuffles it as torch.randperm does.
    Indices, epoch counts and the global generator's state are those of LoaderSource."""

    keyed = False

    def _keys(self, rows, stale):
        """The round's draws from the global generator, for `rows` in order: the seeds of the
        rows that begin an epoch (`stale`, in the same order)."""
        from .sampling import LoaderDraws
        st = self.sampler
        rows = np.asarray(rows, dtype=np.int64)
        seeds = LoaderDraws.round(st.cached[rows] != st.epoch[rows],
                                  st.cursor[rows] + st.b >= st.length[rows])
        return seeds.astype(np.uint32).view(np.int32)

    def _sort(self, stale, n_short):
        """niidmix::torch_randperm: the short rows in one call, the long ones in another, so that a
        call's LDS follows its longest row; no scratch."""
        m, length = len(stale), self.sampler.length
        lists, off = self.tr.dev["sort_lists"], self.tr.dev["perm_off"][1]
        for a, b in ((0, n_short), (n_short, m)):
            if b > a:
                ops.torch_randperm(lists[2, a:b], lists[1, a:b], off[a:b], int(length[stale[a:b]].max()),
                                   self.perm)
                self.last_perm_calls += 1


def source_class(sample, sampling, cached, torch_stream=False):
    """The batch source of a run's mode; graph rounds and sample rounds share them."""
    if sampling and torch_stream:
        return TorchStreamSource
    return CachedSource if sampling and cached else DeviceSource if sampling else LoaderSource
