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
"""
import os

import torch

from . import family, ops
# defined in niidmix.family; the training suites (tests/test_gpu_train*.py) call them as train.<name>
from .family import (fp64_reference, fp64_reference_gn_lenet, gn_lenet_offsets,  # noqa: F401
                     reference_gn_lenet, split_gn_lenet)
from .topology import to_csr

FLAG = "--device-training"
FLAG_GN = "--device-training-gn-lenet"
SCRATCH_FRACTION = 0.4   # of the free HBM, for one GN-LeNet gradient call's scratch


def enabled(params):
    return bool(params.get("algorithm", {}).get("device-training"))


def gn_enabled(params):
    return bool(params.get("algorithm", {}).get("device-training-gn-lenet"))


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
            raise ValueError(f"{FLAG_GN if gn_enabled(params) else FLAG}: node {node['rank']}'s "
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


def check_eligible(nodes, params, topology=None):
    """The refusals that need no GPU (d_sgd.init calls this): raises ValueError naming the flag.
    Returns (K, C) for linear models and, under --device-training-gn-lenet, (Cin, C, F) for
    GN-LeNet.  --clique-gradient / --unbiased-gradient are accepted when `topology` gives their
    averaging lists (grad_plan)."""
    from . import d_sgd
    alg = params["algorithm"]
    gn_flag = gn_enabled(params)
    flag = FLAG_GN if gn_flag else FLAG
    if params["topology"]["name"] == "sample":
        raise ValueError(f"{flag} does not support the 'sample' topology")
    env = os.environ.get("NIIDMIX_DEVICES")
    if env and len([i for i in env.split(",") if i.strip()]) > 1:
        raise ValueError(f"{flag} runs on one device; NIIDMIX_DEVICES lists several")
    if not nodes:
        raise ValueError(f"{flag}: no nodes")
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
    fam.limits(shape, flag, int(alg["batch-size"]))
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

    def __init__(self, nodes, topology, params, device):
        from . import d_sgd
        self.shape = check_eligible(nodes, params, topology)
        self.family = family.family_of(nodes[0]["model"])[0]
        self.flag = FLAG_GN if gn_enabled(params) else FLAG
        self.scratch_budget = None       # bytes of scratch per GN-LeNet gradient call (None:
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
        plan = grad_plan(self.n, topology, params, self.flag)
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
        self.idx_host = torch.zeros(self.n * self.b_max + self.n, dtype=torch.int32).pin_memory()
        self.idx_dev = torch.empty_like(self.idx_host, device=dev)
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
        free, _ = torch.cuda.mem_get_info(self.device)
        if need > 0.8 * free:
            raise RuntimeError(f"{self.flag}: {need / 2**30:.1f} GiB of device buffers ({n_buf} slabs of "
                               f"[{self.n}, {self.p}], the train-sets, scratch) do not fit in "
                               f"{free / 2**30:.1f} GiB of free HBM")

    def _gn_need(self, rows):
        return self.family.grad_scratch_bytes(rows, self.b_max, self.sizes)

    def _cut(self):
        """Rows per call of the gradient kernel: all of them for a family whose calls are not cut,
        else as many as keep the call's scratch within the budget."""
        if not self.family.cut:
            return self.n
        budget = self.scratch_budget
        if budget is None:           # taken once: later rounds see the cached scratch block as used
            if self._free_budget is None:
                self._free_budget = SCRATCH_FRACTION * torch.cuda.mem_get_info(self.device)[0]
            budget = self._free_budget
        k = cut_rows(self.n, self._gn_need, budget)
        if k is None:
            raise RuntimeError(f"{self.flag}: {self._gn_need(1) / 2**30:.2f} GiB of scratch for one "
                               f"row of {self.b_max} samples exceed the budget of "
                               f"{budget / 2**30:.2f} GiB")
        return k

    def _gradient(self, x, bi, bl):
        """Gradient and loss of every row of x on this round's batches."""
        cut = self._cut()
        self.last_calls = 0
        for a in range(0, self.n, cut):
            b = min(self.n, a + cut)
            self.family.grad_rows(x, self.data, self.labels, bi[a:b], bl[a:b], self.rows[a:b],
                                  self.grad, self.loss[a:b], self.sizes)
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

    def round(self, nodes, topology, params, mode):
        """One round of every node; returns ({rank: loss}, {rank: epoch_done})."""
        if topology is not self.topology or id(topology.get("weights")) != self.weights_id:
            self.set_topology(topology)
        batches, epoch_done = draw(nodes, params)
        self._host()
        if not self.fresh or self.version != self.slab.version():
            self.upload()
        nb = self.n * self.b_max
        bi = self.idx_host[:nb].view(self.n, self.b_max).numpy()
        bl = self.idx_host[nb:].numpy()
        for i, idx in enumerate(batches):
            k = idx.numel()
            if k < 1 or k > self.b_max or int(idx.max()) >= self.offsets[i + 1] - self.offsets[i]:
                raise ValueError(f"{self.flag}: node {nodes[i]['rank']} drew a batch its train-set or "
                                 "the batch size does not allow")
            bi[i, :k] = idx.numpy() + self.offsets[i]
            bl[i] = k
        self.idx_dev.copy_(self.idx_host, non_blocking=True)           # one H2D copy
        x, y = self.theta[self.cur], self.theta[1 - self.cur]
        self._gradient(x, self.idx_dev[:nb].view(self.n, self.b_max), self.idx_dev[nb:])
        self._step(x)
        self.mixer(x, out=y, mode=mode)
        self.cur = 1 - self.cur
        loss = self.loss.cpu().tolist()
        self.write_back()
        return {nd["rank"]: float(v) for nd, v in zip(nodes, loss)}, epoch_done
