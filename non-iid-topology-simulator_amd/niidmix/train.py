"""Local training on the device for linear models (`--device-training`) and for GN-LeNet
(`--device-training-gn-lenet`).

The reference trains every simulated node with a Python loop of tiny forward / backward passes on
the CPU (d_sgd.py:186-220), about 98 % of a round at 1000 nodes.  For the reference's own linear
model (setup/model/linear.py: one nn.Linear(K, C), log_softmax, nll_loss) DeviceTrainer keeps the
whole round in HBM instead:

    indices (host, the CPU path's RNG stream) -> one H2D copy
    -> the family's gradient op             gradient and loss of every node, one call for linear
                                            models (niidmix::linear_nll_grad_rows)
    -> niidmix::sgd_step_rows / sgd_momentum_step_rows
    -> Mixer                                 the run's --mixing-mode
    -> losses D2H, parameters D2H into the models (synchronous, every round)

The gradient is not bit-identical to ATen's CPU result (another summation order; within 1e-5 of
the condition-aware bound, tests/test_gpu_train.py), so the path is opt-in; sampling is identical:
each node draws from DataLoader(range(len(train-set)), batch_size, shuffle=True), created and
advanced exactly where the CPU path creates and advances its loader, so the global torch RNG
stream and the samples drawn are those of the CPU path.

The reference's other model, GN-LeNet (setup/model/gn_lenet.py), takes the same round with
niidmix::gnlenet_nll_grad_rows as its gradient op, under a flag of its own,
`--device-training-gn-lenet` (which also sets 'device-training'; the plain flag keeps refusing
GN-LeNet).  The kernel's scratch is about 180 KB per sample, so the row list of a round is cut into
several calls when one call's scratch would exceed a budget (a row's bits do not depend on the
cut).

What depends on the model family -- shapes, the kernels' limits, the sample check, the gradient op
and its scratch, the forward probe -- is niidmix.family's; DeviceTrainer holds a family and its
`sizes` and calls through them.  This module keeps what is about the run: the flags, eligibility,
the averaging lists, sampling, the slabs' padding and the cut of a row list (cut_rows).

Gradient averaging (--clique-gradient, --unbiased-gradient; d_sgd.py:47-94) runs under both flags,
between the gradient op and the mixing, on the lists of niidmix.gradient.build_grad_plan:

    whole cliques            niidmix::grad_segment_mean_sgd_step in place of the step op: the
                             clique's mean gradient and the step of every member in one kernel; a
                             node in no clique is not stepped (clique_segments drops its segment)
    removed clique edges,    GradMean (mix_csr | MEAN) into one more [N, P] slab, then the step op
    neighbourhoods           on the rows the reference steps (GradPlan.stepped)

Either way the round equals, bit for bit, the gradient op followed by the reference's
average_gradients, update_gradients and optimizer.step() on the CPU, then the mixing
(tests/test_gpu_train_gradavg.py).  check_eligible needs the topology for this and refuses, naming
the flag, when the lists cannot be built.

The 'sample' topology (the reference's federated-averaging baseline, d_sgd.py:157-175, :236-250)
runs under a third flag, `--device-training-sample` (it sets 'device-training' too and combines
with the GN-LeNet flag; the other two flags keep refusing 'sample').  DeviceTrainer.sample_round:

    d_sgd.get_sample -> draw() on the active nodes, in the sample's order (inactive nodes draw
                        nothing) -> indices, active rows and `first` flags in the one H2D copy
    -> the family's gradient op over the k active rows (jobs in sample order)
    -> niidmix::sample_step_mean_update      the step of the active rows, their average in sample
                                             order and update_models of every row in one launch,
                                             theta[cur] -> theta[1 - cur]; narrow slabs and small
                                             samples (SAMPLE_FUSED_MIN_COLS, _MIN_SHARE) take the
                                             three ops it restates, which measure faster there
                                             (step op, mix_csr | AVERAGE_ONLY, update_rows)
    -> losses of the active nodes D2H, parameters D2H (synchronous)

A node's first momentum step falls in whichever round first samples it, so the trainer keeps on
the host which rows have stepped (first_flags) and sends the k flags with the indices.  Gradient
averaging does not apply and no Mixer is built (the topology is {'edges': {}, 'weights': []}).

Keeping the CPU path's RNG stream costs N DataLoader draws and the index packing in Python every
round, far more than the device work of a linear model's round.  `--device-sampling` (with any of
the three flags above) gives that stream up for one of the project's own, defined in integers
(niidmix.sampling) and drawn where it is consumed: the host keeps (epoch, cursor) of every row
(sampling.SamplerState: epoch_done and the batch lengths need no copy back), sends them in one
small H2D copy, and niidmix::draw_batches writes the indices and lengths straight into the block
the gradient op reads (batches.DeviceSource, in place of draw and the packing).  No DataLoader is
built, node['train-iterator'] stays None and the global torch RNG is not consumed by sampling; such a run
is sample-for-sample comparable only with other --device-sampling runs of the same seed.

niidmix::draw_batches is stateless -- one workgroup sorts a node's whole epoch on every call -- and
so bounded by what a workgroup sorts in LDS (8192 samples).  `--device-sampling-cached` (with
--device-sampling) keeps the same stream but sorts each epoch once: the trainer owns an int32 cache
of offsets[-1] entries, a node's permutation at its data offset; before a round's draw the rows
whose cache is not their current epoch's (SamplerState.stale: every row in round 0, afterwards the
rows that crossed an epoch) are sorted by niidmix::epoch_perm -- rows of up to 8192 samples in one
call without scratch, longer rows in calls cut by cut_rows to the scratch budget -- and
niidmix::take_batches slices the cache into the index block (batches.CachedSource).  Their lists
travel in the same one H2D copy.  Train-sets up to ops.epoch_perm_max_len() are accepted; for shorter ones
the batches are those of plain --device-sampling, bit for bit.

`--device-sampling-torch-stream` (with --device-sampling; it implies the cache) gives the CPU path's
samples back at that speed: the cache is filled with the permutations the nodes' DataLoaders would
draw.  The host draws the loaders' values from the global torch generator (sampling.LoaderDraws: N
at init(), then per round a seed for every row that begins an epoch and a base seed for every row
whose epoch ends, in one vectorised random_()), and niidmix::torch_randperm restates
torch.randperm's CPU algorithm -- MT19937 and a Fisher-Yates walk, one workgroup per row -- on the
seeds' low 32 bits (batches.TorchStreamSource).  Batches, epoch counts and the global generator's
state are those of the run without --device-sampling; train-sets of up to
ops.torch_randperm_max_len() samples (65536) are accepted, and no run seed is needed.

The linear kernel keeps one row's dz in LDS, so batch-size * C is bounded by ops.MAX_BC.
`--device-training-large-batch` (with --device-training or --device-training-sample, linear models
only) lifts that to ops.MAX_B_SLICED samples: a gradient call whose b_max * C exceeds MAX_BC goes
to niidmix::linear_nll_grad_rows_sliced, which cuts the batch into slices (family.LINEAR.sliced);
every other call keeps the existing op, so a flagged run at an ordinary batch size is the unflagged
run bit for bit.  Under --device-sampling-cached the batch may then be as long as
niidmix::take_batches slices (ops.epoch_perm_max_len()); plain --device-sampling keeps its 8192.
One node (the centralised baseline) is a graph round like any other: the Mixer takes n = 1.

Whatever the mode, a round's indices go up in one H2D copy of one pinned int32 block.  Its lists
and the words a round copies are niidmix.batches.IndexLayout's; what fills it is one of four batch
sources, chosen once per trainer (LoaderSource: draw() and the packing; DeviceSource; CachedSource;
TorchStreamSource),
so the two round methods do not know the sampling mode.
"""
import os

import torch

from . import batches, family, ops
# defined in niidmix.family; the training suites (tests/test_gpu_train*.py) call them as train.<name>
from .family import (fp64_reference, fp64_reference_gn_lenet, gn_lenet_offsets,  # noqa: F401
                     reference_gn_lenet, split_gn_lenet)
from .topology import to_csr

FLAG = "--device-training"
FLAG_GN = "--device-training-gn-lenet"
FLAG_SAMPLE = "--device-training-sample"
FLAG_SAMPLING = "--device-sampling"
FLAG_CACHED = "--device-sampling-cached"
FLAG_LARGE = "--device-training-large-batch"
FLAG_TORCH = "--device-sampling-torch-stream"
SCRATCH_FRACTION = 0.4   # of the free HBM, for one GN-LeNet gradient call's scratch
# When a sample round takes the one-launch step + average + broadcast
# (niidmix::sample_step_mean_update) instead of the three ops it restates: slabs of at least
# SAMPLE_FUSED_MIN_COLS columns (a thread of that kernel walks all rows of its columns, so few
# columns cannot fill the device) and a sample of at least SAMPLE_FUSED_MIN_SHARE of the nodes (the
# launch saves 8 B per sampled node-parameter but streams at about 0.87 of the three kernels'
# rate).  Measured on one MI355X at N = 1000: slower than the sequence at k = 100 for every width
# tried, 0.67 x / 0.81 x its time at k = 1000 and 2^20 columns ("The sample round").
SAMPLE_FUSED_MIN_COLS = 1 << 18
SAMPLE_FUSED_MIN_SHARE = 0.5


def enabled(params):
    return bool(params.get("algorithm", {}).get("device-training"))


def gn_enabled(params):
    return bool(params.get("algorithm", {}).get("device-training-gn-lenet"))


def sample_run(params):
    """A run of the 'sample' topology under --device-training-sample: the round of
    DeviceTrainer.sample_round.  The key alone, on another topology, changes nothing."""
    return bool(params.get("algorithm", {}).get("device-training-sample")) and \
        params.get("topology", {}).get("name") == "sample"


def sampling_enabled(params):
    """--device-sampling: the batches come from niidmix.sampling's stream, drawn on the device."""
    return bool(params.get("algorithm", {}).get("device-sampling"))


def cached_enabled(params):
    """--device-sampling-cached: every epoch's permutation is sorted once and kept in HBM.
    --device-sampling-torch-stream fills the same cache, so it counts as well."""
    return bool(params.get("algorithm", {}).get("device-sampling-cached")) or torch_stream_enabled(params)


def torch_stream_enabled(params):
    """--device-sampling-torch-stream: the cached permutations are the CPU path's own, torch's."""
    return bool(params.get("algorithm", {}).get("device-sampling-torch-stream"))


def large_enabled(params):
    """--device-training-large-batch: linear batches beyond ops.MAX_BC train on the sliced kernels."""
    return bool(params.get("algorithm", {}).get("device-training-large-batch"))


def flag_of(params):
    """The flag a refusal names: GN-LeNet's when set, the sample flag on a sample run."""
    return FLAG_GN if gn_enabled(params) else FLAG_SAMPLE if sample_run(params) else FLAG


def padded_ld(p):
    """Leading dimension of the trainer's [N, P] slabs: P rounded up to 4 floats, so every row is
    16-B aligned and the kernels take their float4 paths when K allows."""
    return (p + 3) // 4 * 4


def index_loader(node, params):
    """The node's loader over sample INDICES: the CPU path's DataLoader (d_sgd._loader) with
    range(len(train-set)) as the dataset -- same sampler, same draws from the global RNG."""
    return iter(torch.utils.data.DataLoader(range(len(node["train-set"])),
                                            batch_size=int(params["algorithm"]["batch-size"]),
                                            shuffle=True))


def draw(nodes, params):
    """One round's batches: per node, in order, the next index batch, then the CPU path's look-ahead
    (d_sgd._peek), epoch count and loader reset (d_sgd.py:198-207).  Returns ([int64 index tensor
    per node], {rank: epoch_done})."""
    from .d_sgd import _peek
    batches, epoch_done = [], {}
    for node in nodes:
        idx = next(node["train-iterator"])
        if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int64 or idx.dim() != 1:
            raise ValueError(f"{flag_of(params)}: node {node['rank']}'s "
                             "train-iterator yields samples, not "
                             "indices: the flag must be set when init() creates the loaders")
        batches.append(idx)
        rest = _peek(node["train-iterator"])
        done = rest is None
        if done:
            node["epoch"] += 1
            node["train-iterator"] = index_loader(node, params)
        else:
            node["train-iterator"] = rest
        epoch_done[node["rank"]] = done
    return batches, epoch_done


def first_flags(stepped, rows):
    """Sample rounds with momentum: per row of `rows`, 1 when it has taken no optimizer step yet
    (torch's SGD clones the gradient into a fresh momentum buffer), else 0; the rows are then
    recorded in the set `stepped`, which the trainer keeps on the host."""
    flags = [int(r not in stepped) for r in rows]
    stepped.update(rows)
    return flags


def grad_plan(n, topology, params, flag):
    """gradient.build_grad_plan for n nodes under --clique-gradient / --unbiased-gradient (clique
    wins when both are set, as in the reference), None without either; every reason it cannot be
    built is a ValueError naming `flag`."""
    from .gradient import build_grad_plan
    alg = params["algorithm"]
    name, key = ("clique-gradient", "cliques") if alg.get("clique-gradient") else \
        ("unbiased-gradient", "neighbourhoods") if alg.get("unbiased-gradient") else (None, None)
    if name is None:
        return None
    if topology is None:
        raise ValueError(f"{flag}: --{name} needs the run's topology, none was given")
    if key not in topology:
        raise ValueError(f"{flag}: --{name} needs a topology with '{key}'")
    try:
        return build_grad_plan(n, topology, params)
    except (ValueError, KeyError, IndexError, TypeError) as e:
        raise ValueError(f"{flag}: --{name}: the averaging lists cannot be built "
                         f"({type(e).__name__}: {e})")


def clique_segments(plan):
    """(seg_ptr, seg_row) of a "clique" plan's cliques alone.  build_grad_plan appends a one-member
    segment for every node in no clique (its gradient mean is its own gradient); the reference does
    not step such a node, so the fused mean + step must not see it."""
    n_seg = len(plan.seg_ptr) - 1 - (plan.n - len(plan.stepped))
    return plan.seg_ptr[:n_seg + 1].copy(), plan.seg_row[:len(plan.stepped)].copy()


def check_sampling(nodes, params):
    """--device-sampling's own refusals, each a ValueError naming the flag: the stream needs the
    run's seed, and one workgroup sorts a node's whole train-set (ops.draw_batches_max_len) --
    under --device-sampling-cached a train-set may have ops.epoch_perm_max_len() samples; the batch
    size stays bounded by the index block's kernel.  --device-sampling-torch-stream draws from the
    global torch generator and needs no seed; its kernel shuffles ops.torch_randperm_max_len()
    samples per node, which bounds the batch too under --device-training-large-batch."""
    if torch_stream_enabled(params):
        return check_torch_stream(nodes, params)
    most = ops.draw_batches_max_len()
    longest = ops.epoch_perm_max_len() if cached_enabled(params) else most
    large = large_enabled(params)
    if large and cached_enabled(params):         # niidmix::take_batches slices batches that long
        most = longest
    seed = params.get("meta", {}).get("seed")
    if not isinstance(seed, int) or isinstance(seed, bool):
        raise ValueError(f"{FLAG_SAMPLING} keys its sample stream by params['meta']['seed'], an "
                         f"integer; got {seed!r}")
    b = int(params["algorithm"]["batch-size"])
    if not 1 <= b <= most:
        raise ValueError(f"{FLAG_SAMPLING}: batch size {b} is not in 1..{most}, the longest batch the "
                         "kernel draws" + (f" ({FLAG_CACHED} slices batches of up to "
                                           f"{ops.epoch_perm_max_len()} samples under {FLAG_LARGE})"
                                           if large and not cached_enabled(params) else ""))
    for nd in nodes:
        ts = nd.get("train-set")
        if ts is not None and len(ts) > longest:
            raise ValueError(f"{FLAG_CACHED if cached_enabled(params) else FLAG_SAMPLING}: node "
                             f"{nd['rank']}'s train-set has {len(ts)} samples, "
                             f"the kernel sorts at most {longest} per node")
        if not 0 <= int(nd["rank"]) < 2 ** 31 or not 0 <= int(nd.get("epoch", 0)) < 2 ** 31 - 1:
            raise ValueError(f"{FLAG_SAMPLING}: node {nd['rank']}'s rank or epoch is outside int32")


def check_torch_stream(nodes, params):
    """check_sampling under --device-sampling-torch-stream; the refusals name that flag."""
    longest = ops.torch_randperm_max_len()
    most = longest if large_enabled(params) else ops.draw_batches_max_len()
    b = int(params["algorithm"]["batch-size"])
    if not 1 <= b <= most:
        raise ValueError(f"{FLAG_TORCH}: batch size {b} is not in 1..{most}, the longest batch the "
                         "kernel draws" + ("" if large_enabled(params) else
                                           f" ({longest} under {FLAG_LARGE})"))
    for nd in nodes:
        ts = nd.get("train-set")
        if ts is not None and len(ts) > longest:
            raise ValueError(f"{FLAG_TORCH}: node {nd['rank']}'s train-set has {len(ts)} samples, the "
                             f"kernel shuffles at most {longest} per node")
        if not 0 <= int(nd.get("epoch", 0)) < 2 ** 31 - 1:
            raise ValueError(f"{FLAG_TORCH}: node {nd['rank']}'s epoch is outside int32")


def check_eligible(nodes, params, topology=None):
    """The refusals that need no GPU (d_sgd.init calls this): raises ValueError naming the flag
    (--device-sampling's are check_sampling's, and that it needs one of the training flags;
    --device-sampling-cached needs --device-sampling).
    Returns (K, C) for linear models and, under --device-training-gn-lenet, (Cin, C, F) for
    GN-LeNet.  --clique-gradient / --unbiased-gradient are accepted when `topology` gives their
    averaging lists (grad_plan).  The 'sample' topology is accepted under --device-training-sample
    only; such a run ignores the two gradient-averaging flags, as the reference's sample branch
    does, and needs nothing of `topology`."""
    from . import d_sgd
    alg = params["algorithm"]
    if torch_stream_enabled(params) and not sampling_enabled(params):
        raise ValueError(f"{FLAG_TORCH} shuffles {FLAG_SAMPLING}'s batches as torch does: it needs "
                         f"{FLAG_SAMPLING}")
    if cached_enabled(params) and not sampling_enabled(params):
        raise ValueError(f"{FLAG_CACHED} caches the permutations of {FLAG_SAMPLING}'s stream: it needs "
                         f"{FLAG_SAMPLING}")
    if sampling_enabled(params) and not enabled(params):
        raise ValueError(f"{FLAG_SAMPLING} draws the batches of a device-training round: it needs one "
                         f"of {FLAG}, {FLAG_GN} or {FLAG_SAMPLE}")
    gn_flag = gn_enabled(params)
    flag = flag_of(params)
    sample = sample_run(params)
    large = large_enabled(params)
    if large and not enabled(params):
        raise ValueError(f"{FLAG_LARGE} lifts the batch limit of a linear model's device-training "
                         f"round: it needs {FLAG} or {FLAG_SAMPLE}")
    if large and gn_flag:
        raise ValueError(f"{FLAG_LARGE} is for linear models: GN-LeNet's kernels ({FLAG_GN}) have no "
                         "such batch limit")
    if params["topology"]["name"] == "sample" and not sample:
        raise ValueError(f"{flag} does not support the 'sample' topology: it trains on the device "
                         f"under {FLAG_SAMPLE}")
    env = os.environ.get("NIIDMIX_DEVICES")
    if env and len([i for i in env.split(",") if i.strip()]) > 1:
        raise ValueError(f"{flag} runs on one device; NIIDMIX_DEVICES lists several")
    if not nodes:
        raise ValueError(f"{flag}: no nodes")
    if sampling_enabled(params):
        check_sampling(nodes, params)
    if sample:
        size = params["topology"].get("sample-size")
        if not isinstance(size, int) or not 1 <= size <= len(nodes):
            raise ValueError(f"{flag}: sample-size {size!r} is not in 1..{len(nodes)}")
    else:
        grad_plan(len(nodes), topology, params, flag)
    fam, shape = family.family_of(nodes[0]["model"]) or (None, None)
    gn = fam is family.GN_LENET
    lr, mom = float(alg["learning-rate"]), d_sgd._momentum(params)
    if gn and not gn_flag:
        raise ValueError(f"{flag} trains linear models only; GN-LeNet models train on the "
                         f"device under {FLAG_GN}")
    for nd in nodes:
        if not gn and (fam is None or fam.shape(nd["model"]) != shape):
            raise ValueError(f"{flag} needs models whose parameters are exactly a [C, K] weight and "
                             f"a [C] bias" + (", or exactly GN-LeNet's 14 tensors" if gn_flag else "") +
                             f", the same on every node (node {nd['rank']} differs)")
        opt = nd.get("optimizer")
        ps = list(nd["model"].parameters())
        if not d_sgd._plugin_sgd(opt, lr, mom) or len(opt.param_groups[0]["params"]) != len(ps) or \
                any(a is not b for a, b in zip(opt.param_groups[0]["params"], ps)):
            raise ValueError(f"{flag} needs the plugin's SGD optimizer (niidmix.d_sgd.optimizer) at "
                             f"the run's learning rate and momentum (node {nd['rank']})")
    for nd in nodes:
        if gn and fam.shape(nd["model"]) != shape:
            raise ValueError(f"{flag} needs models whose parameters are exactly GN-LeNet's 14 "
                             f"tensors, the same on every node (node {nd['rank']} differs)")
    fam.limits(shape, FLAG_LARGE if large else flag, int(alg["batch-size"]), large)
    for nd in nodes:
        ts = nd.get("train-set")         # an empty set is DeviceTrainer's refusal, and so are a
        if gn and ts is not None and len(ts):                   # linear model's samples
            fam.sizes(tuple(torch.as_tensor(ts[0][0]).shape), shape, flag,
                      f"node {nd['rank']}'s train-set")
    return shape


def cut_rows(n, need, budget):
    """Rows per call such that need(rows) <= budget: n when everything fits, else halved until it
    does; None when one row does not fit.  The one cut: niidmix.evaluate's job lists use it too."""
    if need(1) > budget:
        return None
    k = n
    while need(k) > budget:
        k = (k + 1) // 2
    return k


class DeviceTrainer:
    """Data, parameters, gradients (and momentum) of one node list in HBM, and the round above."""

    kind = property(lambda self: self.family.kind)       # "linear" / "gn-lenet", read-only
    last_perm_jobs = property(lambda self: self.source.last_perm_jobs)       # batches.CachedSource's, of
    last_perm_calls = property(lambda self: self.source.last_perm_calls)     # the last round (tests)

    def __init__(self, nodes, topology, params, device):
        from . import d_sgd
        self.shape = check_eligible(nodes, params, topology)
        self.family = family.family_of(nodes[0]["model"])[0]
        self.flag = flag_of(params)
        self.sample = sample_run(params)     # fixed for the trainer's life (d_sgd._trainer)
        self.sampling = sampling_enabled(params)     # and so are these three
        self.cached = cached_enabled(params)
        self.torch_stream = torch_stream_enabled(params)
        self.large = large_enabled(params)           # batches beyond ops.MAX_BC: the sliced op
        self.scratch_budget = None      # bytes of scratch per GN-LeNet gradient call (None:
        self.last_calls = 0              # SCRATCH_FRACTION of the free HBM); calls of the last round
        self.sizes = None                # the kernel's size arguments (family.sizes), set by _materialise
        self._free_budget = None         # the default budget, measured before the first gradient call
        self.c = self.shape[1]
        self.p = self.family.P(self.shape)
        self.ld = padded_ld(self.p)
        self.n = len(nodes)
        self.device = torch.device(device)
        self.models = [nd["model"] for nd in nodes]
        self.b_max = int(params["algorithm"]["batch-size"])
        self.lr = float(params["algorithm"]["learning-rate"])
        self.momentum = d_sgd._momentum(params)
        if self.momentum != 0.0 and d_sgd._momentum_state(nodes) != "none":
            raise ValueError(f"{self.flag} was switched on while the CPU optimizers hold momentum "
                             "buffers: handing them to the device mid-run is not supported")
        self.params = params
        # a sample run ignores --clique-gradient / --unbiased-gradient (d_sgd.py:236-250)
        plan = None if self.sample else grad_plan(self.n, topology, params, self.flag)
        self.grad_kind = plan.kind if plan is not None else None     # fixed by params for the run
        # the per-row kinds average into a slab of their own; the clique kind needs none
        self.n_buf = 3 + (self.momentum != 0.0) + (self.grad_kind in ("clique-removed", "unbiased"))
        xs, ys, self.offsets = self._materialise(nodes)
        self._check_fit(xs)
        dev = self.device
        self.data = xs.to(dev)
        self.labels = ys.to(dev)
        slabs = [torch.zeros((self.n, self.ld), dtype=torch.float32, device=dev)
                 for _ in range(self.n_buf)]
        self.theta = [s[:, :self.p] for s in slabs[:2]]      # ping-pong: mixing is out-of-place
        self.grad = slabs[2][:, :self.p]
        self.mbuf = slabs[3][:, :self.p] if self.momentum != 0.0 else None
        self.gavg = slabs[-1][:, :self.p] if self.grad_kind in ("clique-removed", "unbiased") else None
        self.cur = 0
        self.mom_steps = 0
        self.rows = torch.arange(self.n, dtype=torch.int32, device=dev)
        self.loss = torch.empty(self.n, dtype=torch.float32, device=dev)
        # one round's indices, one H2D copy: batches.IndexLayout's lists, filled by the mode's source
        self.layout = batches.IndexLayout(self.n, self.b_max, self.sample, self.sampling, self.cached)
        self.idx_host = torch.zeros(self.layout.words, dtype=torch.int32).pin_memory()
        self.idx_dev = torch.empty_like(self.idx_host, device=dev)
        self.dev = {name: self.layout.view(self.idx_dev, name) for name in self.layout.spans}
        self.source = batches.source_class(self.sample, self.sampling, self.cached,
                                                self.torch_stream)(self, nodes)
        self.stepped_rows = set()     # sample rounds: rows that have taken an optimizer step
        self.last_first = []          # the `first` flags of the last sample round (tests)
        self._avg = None              # sample rounds, three-op sequence: the CSR row and the average
        self.sample_fused = None      # the last sample round took the one launch (sample_round)
        self.fresh = False            # the device parameters are the models' current values
        self.version = None           # NodeSlab.version() the device copy corresponds to
        self.slab = None
        self.param_uploads = 0
        self.mixer = None
        self.set_topology(topology)
        self._probe(nodes, params)

    # -------------------------------------------------------------------------------------------
    def _materialise(self, nodes):
        xs, ys, offsets = [], [], [0]
        for nd in nodes:
            ts = nd["train-set"]
            items = [ts[j] for j in range(len(ts))]
            if not items:
                raise ValueError(f"{self.flag}: node {nd['rank']} has an empty train-set")
            x = torch.stack([torch.as_tensor(s[0]) for s in items])
            sizes = self.family.sizes(tuple(x.shape[1:]), self.shape, self.flag,
                                      f"node {nd['rank']}'s train-set")
            if self.sizes not in (None, sizes):
                raise ValueError(f"{self.flag}: node {nd['rank']}'s samples are "
                                 f"{tuple(x.shape[1:])}, earlier nodes' {self.sizes[:-1]}")
            self.sizes = sizes
            x = x.reshape(len(items), -1)
            y = torch.as_tensor([int(s[1]) for s in items], dtype=torch.int64)
            if int(y.min()) < 0 or int(y.max()) >= self.c:
                raise ValueError(f"{self.flag}: node {nd['rank']} has a label outside [0, {self.c})")
            xs.append(x.to(torch.float32))
            ys.append(y.to(torch.int32))
            offsets.append(offsets[-1] + len(items))
        if offsets[-1] >= 2 ** 31:
            raise ValueError(f"{self.flag}: {offsets[-1]} samples exceed int32 indices")
        return torch.cat(xs).contiguous(), torch.cat(ys).contiguous(), offsets

    def _check_fit(self, xs):
        """ResidentRound.fits-style arithmetic: slabs, data and the kernel's scratch against the
        free HBM.  No fit is an error: there is no silent CPU fallback under an explicit flag."""
        n_buf = self.n_buf
        need = n_buf * self.n * self.ld * 4 + xs.numel() * 4
        # where calls are cut, one row's scratch at least: _cut sizes the calls every round
        need += self._gn_need(1 if self.family.cut else self.n)
        if self.cached:      # the permutation cache, and the sort's scratch for the longest row alone
            longest = max(b - a for a, b in zip(self.offsets, self.offsets[1:]))
            need += self.offsets[-1] * 4
            need += 0 if self.torch_stream else ops.epoch_perm_scratch_bytes(1, longest)
        free, _ = torch.cuda.mem_get_info(self.device)
        if need > 0.8 * free:
            raise RuntimeError(f"{self.flag}: {need / 2**30:.1f} GiB of device buffers ({n_buf} slabs of "
                               f"[{self.n}, {self.p}], the train-sets, scratch) do not fit in "
                               f"{free / 2**30:.1f} GiB of free HBM")

    def _gn_need(self, rows):
        return self.family.grad_scratch_bytes(rows, self.b_max, self.sizes, self.large)

    def _budget(self):
        """Bytes of scratch one call may take: scratch_budget when set, else SCRATCH_FRACTION of the
        HBM that was free before the first such call."""
        if self.scratch_budget is not None:
            return self.scratch_budget
        if self._free_budget is None:    # taken once: later rounds see the cached scratch block as used
            self._free_budget = SCRATCH_FRACTION * torch.cuda.mem_get_info(self.device)[0]
        return self._free_budget

    def _cut(self, n):
        """Rows per call of the gradient kernel over n jobs: all of them for a family whose calls
        are not cut, else as many as keep the call's scratch within the budget."""
        if not self.family.cut:
            return n
        budget = self._budget()
        k = cut_rows(n, self._gn_need, budget)
        if k is None:
            raise RuntimeError(f"{self.flag}: {self._gn_need(1) / 2**30:.2f} GiB of scratch for one "
                               f"row of {self.b_max} samples exceed the budget of "
                               f"{budget / 2**30:.2f} GiB")
        return k

    def _gradient(self, x, rows=None):
        """Gradient and loss of the rows `rows` of x (default: every row) on this round's batches
        (the index block's, where the batch source put them), one job per row in the list's order:
        job j's gradient goes to row rows[j] of self.grad, its loss to self.loss[j]."""
        rows = self.rows if rows is None else rows
        n = rows.numel()
        bi, bl = self.dev["indices"], self.dev["lengths"]
        cut = self._cut(n)
        self.last_calls = 0
        for a in range(0, n, cut):
            b = min(n, a + cut)
            self.family.grad_rows(x, self.data, self.labels, bi[a:b], bl[a:b], rows[a:b],
                                  self.grad, self.loss[a:b], self.sizes, self.large)
            self.last_calls += 1

    def _step(self, x):
        """The optimizer step of the round on the parameters x, after the gradient averaging the
        run asks for.  Whole cliques: the mean and the step of every clique member in one kernel
        (a node in no clique is not stepped, as in the reference); per-row lists: the mean into a
        slab of its own, then the step op on the rows the reference steps.  `first` is right
        because every stepped row steps every round."""
        first = self.mom_steps == 0
        if self.grad_kind == "clique":
            ops.grad_segment_mean_sgd_step(x, self.grad, self.mbuf, *self.segments, -self.lr,
                                           self.momentum, first)
        else:
            g, rows = self.grad, self.rows
            if self.gmean is not None:
                g, rows = self.gmean(self.grad, out=self.gavg), self.step_rows
            if self.momentum != 0.0:
                ops.sgd_momentum_step_rows(x, g, self.mbuf, rows, -self.lr, self.momentum, first)
            else:
                ops.sgd_step_rows(x, g, rows, -self.lr)
        if self.momentum != 0.0:
            self.mom_steps += 1

    def _probe(self, nodes, params):
        """The family's gradient probe on node 0's first samples."""
        ts = nodes[0]["train-set"]
        nb = min(family.PROBE_SAMPLES, len(ts), self.b_max)
        items = [ts[j] for j in range(nb)]
        x = torch.stack([torch.as_tensor(s[0]) for s in items])
        y = torch.as_tensor([int(s[1]) for s in items], dtype=torch.int64)
        self.family.probe_grad(self.models[0], x, y, params, self.device, self.sizes, self.flag, "node 0's")

    # -------------------------------------------------------------------------------------------
    def owns(self, nodes):
        return len(nodes) == self.n and all(nd["model"] is m for nd, m in zip(nodes, self.models))

    def holds(self, nodes):
        """Any of the nodes' models is one of the trainer's."""
        mine = {id(m) for m in self.models}
        return any(id(nd["model"]) in mine for nd in nodes)

    def set_topology(self, topology):
        if self.sample:              # {'edges': {}, 'weights': []}: no graph, no Mixer, no lists
            self.stepped = self.segments = self.gmean = self.step_rows = None
            self.topology = topology
            self.weights_id = id(topology.get("weights")) if topology is not None else None
            return
        csr = to_csr(topology)
        if csr.n != self.n:
            raise ValueError(f"topology has {csr.n} nodes, {self.n} models given")
        plan = grad_plan(self.n, topology, self.params, self.flag)
        if (plan.kind if plan is not None else None) != self.grad_kind:
            raise ValueError(f"{self.flag}: the gradient averaging changed from {self.grad_kind} to "
                             f"{plan.kind if plan is not None else None} during the run")
        stepped = None if plan is None else frozenset(plan.stepped)
        if self.mom_steps and stepped != self.stepped:
            raise ValueError(f"{self.flag}: the new topology changes which nodes take the optimizer "
                             "step while momentum buffers live on the device: not supported")
        torch.cuda.synchronize(self.device)      # nothing reads the old descriptors any more
        self.mixer = ops.Mixer(csr=csr, cliques=topology.get("cliques"), device=self.device)
        self.stepped = stepped
        self.segments = self.gmean = self.step_rows = None
        if self.grad_kind == "clique":
            self.segments = tuple(torch.from_numpy(a).to(self.device) for a in clique_segments(plan))
        elif plan is not None:
            from .gradient import GradMean
            self.gmean = GradMean(plan, self.device)
            self.step_rows = torch.tensor(plan.stepped, dtype=torch.int32, device=self.device)
        self.topology = topology
        self.weights_id = id(topology.get("weights"))

    def _host(self):
        """The pinned [N, P] host slab the models' parameters are views of (niidmix.slab.NodeSlab;
        made again when a model's parameters were moved off it): both copies are one transfer."""
        from .slab import NodeSlab
        if self.slab is None or not self.slab.owns(self.models):
            self.slab = NodeSlab(self.models)
            self.fresh = False
        return self.slab.host

    def upload(self):
        self.theta[self.cur].copy_(self._host())
        self.param_uploads += 1
        self.fresh = True
        self.version = self.slab.version()

    def current(self):
        """The device parameters [N, P] when they are the models' current values (the test round()
        makes before it decides to upload), else None.  Readers such as
        niidmix.evaluate.DeviceEvaluator use them in place: no upload."""
        if not self.fresh or self.slab is None or not self.slab.owns(self.models) or \
                self.version != self.slab.version():
            return None
        return self.theta[self.cur]

    def write_back(self):
        self._host().copy_(self.theta[self.cur])     # D2H, synchronous: the models are current

    def _current_params(self):
        """Makes the device parameters the models' current values (an upload when they are not).
        Returns the slab that holds them and the one the round writes."""
        self._host()
        if not self.fresh or self.version != self.slab.version():
            self.upload()
        return self.theta[self.cur], self.theta[1 - self.cur]

    def _finish(self, nodes, k):
        """The end of a round, whose result is in the other slab: the losses of its k jobs D2H, the
        parameters back into the models (synchronous).  Returns {rank: loss} of `nodes`, the jobs'
        nodes in order."""
        self.cur = 1 - self.cur
        loss = self.loss[:k].cpu().tolist()
        self.write_back()
        return {nd["rank"]: float(v) for nd, v in zip(nodes, loss)}

    def _sample_sequence(self, x, y, active, lists, n_first):
        """Step, average and broadcast of a sample round as the three ops in sequence (x is
        stepped in place): what niidmix::sample_step_mean_update restates in one launch."""
        k = active.numel()
        if self.momentum != 0.0:
            for rows, first in ((lists[:n_first], True), (lists[n_first:], False)):
                if rows.numel():
                    ops.sgd_momentum_step_rows(x, self.grad, self.mbuf, rows, -self.lr, self.momentum, first)
        else:
            ops.sgd_step_rows(x, self.grad, active, -self.lr)
        if self._avg is None or self._avg[0] != k:
            import numpy as np
            self._avg = (k, torch.tensor([0, k], dtype=torch.int64, device=self.device),
                         torch.full((k,), float(np.float32(1.0 / k)), dtype=torch.float32, device=self.device),
                         torch.empty((1, self.ld), dtype=torch.float32, device=self.device)[:, :self.p])
        _, row_ptr, val, avg = self._avg
        ops.mix_csr(x, row_ptr, active, val, avg, ops.EXACT | ops.AVERAGE_ONLY)
        ops.update_rows(x, avg[0], y)

    def sample_round(self, nodes, active, params):
        """One round of the 'sample' topology (d_sgd.py:236-250): the nodes `active` (d_sgd.get_sample,
        in its order) draw, train and step; their uniform average then replaces every node's model.
        Returns ({rank: loss}, {rank: epoch_done}) of the active nodes.  Inactive nodes draw
        nothing and their momentum buffers are not touched; a node's first momentum step falls in
        the round that first samples it (first_flags)."""
        if not self.sample:
            raise ValueError(f"{self.flag}: this trainer was not built for a sample run")
        pos = {id(nd): i for i, nd in enumerate(nodes)}
        rows = [pos[id(nd)] for nd in active]
        k = len(rows)
        if k < 1 or len(set(rows)) != k:
            raise ValueError(f"{self.flag}: a sample of {k} nodes with {len(set(rows))} distinct ones")
        first = self.last_first = first_flags(self.stepped_rows, rows)
        order = [r for r, f in zip(rows, first) if f] + [r for r, f in zip(rows, first) if not f]
        self.layout.view(self.idx_host, "sample_tail")[:, :k] = torch.tensor([rows, first, order])
        epoch_done = self.source.fill(active, rows, params)     # the one H2D copy, the tail in it
        x, y = self._current_params()
        dev = self.dev["sample_tail"]
        self._gradient(x, dev[0, :k])
        self.sample_fused = self.ld >= SAMPLE_FUSED_MIN_COLS and k >= SAMPLE_FUSED_MIN_SHARE * self.n
        if self.sample_fused:
            mom = self.momentum != 0.0
            ops.sample_step_mean_update(x, y, self.grad, self.mbuf, dev[0, :k], dev[1, :k] if mom else None,
                                        -self.lr, self.momentum)
        else:
            self._sample_sequence(x, y, dev[0, :k], dev[2, :k], sum(first))
        if self.momentum != 0.0:
            self.mom_steps += 1
        return self._finish(active, k), epoch_done

    def round(self, nodes, topology, params, mode):
        """One round of every node; returns ({rank: loss}, {rank: epoch_done})."""
        if self.sample:
            raise ValueError(f"{self.flag}: a sample run's rounds are sample_round's")
        if topology is not self.topology or id(topology.get("weights")) != self.weights_id:
            self.set_topology(topology)
        epoch_done = self.source.fill(nodes, None, params)      # the one H2D copy
        x, y = self._current_params()
        self._gradient(x)
        self._step(x)
        self.mixer(x, out=y, mode=mode)
        return self._finish(nodes, self.n), epoch_done
