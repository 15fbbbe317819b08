"""Local training on the device for linear models (`--device-training`) and for GN-LeNet
(`--device-training-gn-lenet`).

The reference trains every simulated node with a Python loop of tiny forward / backward passes on
the CPU (d_sgd.py:186-220), about 98 % of a round at 1000 nodes.  For the reference's own linear
model (setup/model/linear.py: one nn.Linear(K, C), log_softmax, nll_loss) DeviceTrainer keeps the
whole round in HBM instead:

    indices (host, the CPU path's RNG stream) -> one H2D copy
    -> niidmix::linear_nll_grad_rows        gradient and loss of every node, one call
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
import copy
import os

import torch
import torch.nn.functional as F

from . import ops
from .topology import to_csr

FLAG = "--device-training"
FLAG_GN = "--device-training-gn-lenet"
PROBE_SAMPLES = 8
# the kernels' limits (include/niidmix.h)
MAX_C = 1024
MAX_BC = 32768
GN_MAX_CIN, GN_MIN_HW, GN_MAX_HW = 4, 15, 64
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


def linear_shape(model):
    """(K, C) when the model's parameters are exactly a [C, K] weight then a [C] bias, else None."""
    ps = list(model.parameters())
    if len(ps) != 2 or ps[0].dim() != 2 or ps[1].dim() != 1 or ps[1].shape[0] != ps[0].shape[0]:
        return None
    if any(q.dtype != torch.float32 or not q.requires_grad for q in ps):
        return None
    return int(ps[0].shape[1]), int(ps[0].shape[0])


def gn_lenet_shape(model):
    """(Cin, C, F) when the model's parameters are exactly GN-LeNet's 14 tensors in registration
    order (include/niidmix.h, niidmix_gnlenet_eval_rows_f32), fp32 and trainable, else None."""
    ps = list(model.parameters())
    if len(ps) != 14 or ps[0].dim() != 4 or ps[12].dim() != 2:
        return None
    if any(q.dtype != torch.float32 or not q.requires_grad for q in ps):
        return None
    cin, (c, f) = int(ps[0].shape[1]), (int(v) for v in ps[12].shape)
    want = [(32, cin, 5, 5), (32,), (32,), (32,), (32, 32, 5, 5), (32,), (32,), (32,),
            (64, 32, 5, 5), (64,), (64,), (64,), (c, f), (c,)]
    if [tuple(q.shape) for q in ps] != want or cin < 1 or f < 64 or f % 64:
        return None
    return cin, c, f


def gn_lenet_offsets(cin, c, f):
    """Start of each of the 14 tensors in a flattened row, and P at the end (15 values)."""
    sizes = [800 * cin, 32, 32, 32, 25600, 32, 32, 32, 51200, 64, 64, 64, c * f, c]
    out = [0]
    for v in sizes:
        out.append(out[-1] + v)
    return out


def _check_gn_lenet(nodes, shape, flag):
    """check_eligible's GN-LeNet part: one shape on every node, the kernel's limits, and samples
    that are [Cin, H, W] images giving the classifier's F.  Returns (Cin, C, F)."""
    for nd in nodes:
        if gn_lenet_shape(nd["model"]) != shape:
            raise ValueError(f"{flag} needs models whose parameters are exactly GN-LeNet's 14 "
                             f"tensors, the same on every node (node {nd['rank']} differs)")
    cin, c, f = shape
    if c > MAX_C:
        raise ValueError(f"{flag}: C = {c} exceeds the kernel's limit (C <= {MAX_C})")
    if cin > GN_MAX_CIN:
        raise ValueError(f"{flag}: {cin} input channels exceed the kernel's limit "
                         f"(Cin <= {GN_MAX_CIN})")
    for nd in nodes:
        ts = nd.get("train-set")
        if ts is None or len(ts) == 0:
            continue                                    # an empty set is DeviceTrainer's refusal
        sample_sizes(tuple(torch.as_tensor(ts[0][0]).shape), shape, flag,
                     f"node {nd['rank']}'s train-set")
    return shape


def sample_sizes(sh, shape, flag, what):
    """(Cin, H, W, C) for samples of shape `sh` under a GN-LeNet of shape (Cin, C, F); ValueError
    naming `flag` when the kernels do not take them."""
    cin, c, f = shape
    if len(sh) != 3 or sh[0] != cin:
        raise ValueError(f"{flag}: the samples of {what} have shape {tuple(sh)}, GN-LeNet takes "
                         f"[{cin}, H, W]")
    h, w = int(sh[1]), int(sh[2])
    if not (GN_MIN_HW <= h <= GN_MAX_HW and GN_MIN_HW <= w <= GN_MAX_HW):
        raise ValueError(f"{flag}: samples of {h} x {w} in {what}: the kernel takes "
                         f"{GN_MIN_HW} <= H, W <= {GN_MAX_HW}")
    got = ops.gnlenet_sizes(cin, h, w, c)[0]
    if got != f:
        raise ValueError(f"{flag}: samples of shape {tuple(sh)} in {what} give GN-LeNet {got} "
                         f"features, the model's classifier takes F = {f}")
    return cin, h, w, c


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
    shape = linear_shape(nodes[0]["model"])
    gn_shape = gn_lenet_shape(nodes[0]["model"]) if shape is None else None
    lr, mom = float(alg["learning-rate"]), d_sgd._momentum(params)
    for nd in nodes:
        if gn_shape is not None and not gn_flag:
            raise ValueError(f"{flag} trains linear models only; GN-LeNet models train on the "
                             f"device under {FLAG_GN}")
        if gn_shape is None and (shape is None or linear_shape(nd["model"]) != shape):
            raise ValueError(f"{flag} needs models whose parameters are exactly a [C, K] weight and "
                             f"a [C] bias" + (", or exactly GN-LeNet's 14 tensors" if gn_flag else "") +
                             f", the same on every node (node {nd['rank']} differs)")
        opt = nd.get("optimizer")
        ps = list(nd["model"].parameters())
        if not d_sgd._plugin_sgd(opt, lr, mom) or len(opt.param_groups[0]["params"]) != len(ps) or \
                any(a is not b for a, b in zip(opt.param_groups[0]["params"], ps)):
            raise ValueError(f"{flag} needs the plugin's SGD optimizer (niidmix.d_sgd.optimizer) at "
                             f"the run's learning rate and momentum (node {nd['rank']})")
    if gn_shape is not None:
        return _check_gn_lenet(nodes, gn_shape, flag)
    k, c = shape
    b = int(alg["batch-size"])
    if c > MAX_C or b * c > MAX_BC:
        raise ValueError(f"{flag}: C = {c}, batch-size * C = {b * c} exceed the kernel's limits "
                         f"(C <= {MAX_C}, batch-size * C <= {MAX_BC})")
    return k, c


def _flat_params(models):
    return torch.stack([torch.cat([q.detach().reshape(-1) for q in m.parameters()]) for m in models])


def fp64_reference(w, b, x, y):
    """Loss, gradient and the condition-aware bound A of one batch in float64 (torch CPU):
    (loss64, g64 [P], A [P]) for W [C, K], b [C], x [B, K], y [B] -- the yardstick of the forward
    probe and of tests/test_gpu_train.py."""
    w, b, x = w.double(), b.double(), x.double()
    z = x @ w.t() + b
    lp = F.log_softmax(z, 1)
    n = x.shape[0]
    loss = -lp[torch.arange(n), y].mean()
    p = lp.exp()
    oh = F.one_hot(y, w.shape[0]).double()
    dz = (p - oh) / n
    g = torch.cat([(dz.t() @ x).reshape(-1), dz.sum(0)])
    az = (p + oh) / n
    a = torch.cat([(az.t() @ x.abs()).reshape(-1), az.sum(0)])
    return loss, g, a


def probe_forward(model, x, y, params, device, flag, whose="the"):
    """`forward` cannot be inspected: require that model.forward + nll_loss + backward on the CPU
    agree with the gradient kernel on the samples x (as the model takes them) with labels y, under
    the tests' tolerance (both are within 1e-5 A of the float64 result, hence within 2e-5 A of each
    other).  Shared by DeviceTrainer and niidmix.evaluate.DeviceEvaluator; raises ValueError naming
    `flag`."""
    k, c = linear_shape(model)
    p, nb = c * k + c, int(x.shape[0])
    mdl = copy.deepcopy(model)
    for q in mdl.parameters():
        q.grad = None
    loss = F.nll_loss(mdl.forward(x, params), y)
    loss.backward()
    g_cpu = torch.cat([q.grad.reshape(-1) for q in mdl.parameters()])
    dev = torch.device(device)
    theta = torch.zeros((1, padded_ld(p)), dtype=torch.float32, device=dev)[:, :p]
    theta.copy_(_flat_params([mdl]))
    grad = torch.zeros((1, padded_ld(p)), dtype=torch.float32, device=dev)[:, :p]
    out = torch.empty(1, dtype=torch.float32, device=dev)
    bi = torch.arange(nb, dtype=torch.int32, device=dev).reshape(1, nb)
    bl = torch.tensor([nb], dtype=torch.int32, device=dev)
    xf = x.reshape(nb, -1).to(torch.float32)
    ops.linear_nll_grad_rows(theta, xf.contiguous().to(dev), y.to(torch.int32).to(dev), bi, bl,
                             torch.zeros(1, dtype=torch.int32, device=dev), grad, out, k, c)
    w, b = [q.detach() for q in mdl.parameters()]
    l64, _, a = fp64_reference(w, b, xf, y)
    dg = (grad[0].cpu().double() - g_cpu.double()).abs()
    loss = loss.detach()
    dl = abs(float(out[0]) - float(loss))
    if not bool((dg <= 2e-5 * a).all()) or not dl <= 2e-5 * max(abs(float(l64)), 1.0):
        raise ValueError(
            f"{flag}: the model's forward is not log_softmax(Linear(x.view(-1, K))): on {whose} "
            f"first {nb} samples the kernel's loss {float(out[0]):.6g} / gradient differ from "
            f"forward + nll_loss + backward on the CPU (loss {float(loss):.6g}, worst gradient "
            f"ratio {float((dg / a.clamp_min(1e-300)).max()):.3g} of the bound)")


def gn_lenet_forward(ts, x):
    """GN-LeNet's forward on its 14 tensors `ts` (any dtype): log-probabilities [B, C] of x
    [B, Cin, H, W] (include/niidmix.h, niidmix_gnlenet_eval_rows_f32)."""
    h = F.max_pool2d(F.conv2d(x, ts[0], ts[1], padding=2), 3, 2)
    h = F.relu(F.group_norm(h, 2, ts[2], ts[3], 1e-5))
    h = F.group_norm(F.conv2d(h, ts[4], ts[5], padding=2), 2, ts[6], ts[7], 1e-5)
    h = F.relu(F.max_pool2d(h, 3, 2))
    h = F.group_norm(F.conv2d(h, ts[8], ts[9], padding=2), 2, ts[10], ts[11], 1e-5)
    h = F.relu(F.max_pool2d(h, 3, 2))
    return F.log_softmax(F.linear(h.flatten(1), ts[12], ts[13]), 1)


def split_gn_lenet(theta_row, cin, hw):
    """The 14 tensors (views) of a flattened GN-LeNet row for samples [cin, *hw]; C follows from
    the row's length."""
    f = ops.gnlenet_sizes(cin, hw[0], hw[1], 1)[0]
    p = int(theta_row.numel())
    c, rem = divmod(p - 800 * cin - 77184, f + 1)
    if c < 1 or rem:
        raise ValueError(f"a row of {p} values is no GN-LeNet for samples of [{cin}, {hw[0]}, {hw[1]}]")
    off = gn_lenet_offsets(cin, c, f)
    shapes = [(32, cin, 5, 5), (32,), (32,), (32,), (32, 32, 5, 5), (32,), (32,), (32,),
              (64, 32, 5, 5), (64,), (64,), (64,), (c, f), (c,)]
    return [theta_row[off[i]:off[i + 1]].reshape(sh) for i, sh in enumerate(shapes)]


def reference_gn_lenet(theta_row, x, y, dtype):
    """(loss, gradient [P]) of F.nll_loss(forward(x), y) by torch autograd on the CPU in `dtype`,
    over the functional forward; theta_row [P], x [B, Cin, H, W], y [B] int64."""
    th = theta_row.detach().to(dtype).clone().requires_grad_(True)
    ts = split_gn_lenet(th, int(x.shape[1]), (int(x.shape[2]), int(x.shape[3])))
    loss = F.nll_loss(gn_lenet_forward(ts, x.to(dtype)), y.to(torch.int64))
    (g,) = torch.autograd.grad(loss, th)
    return loss.detach(), g


def fp64_reference_gn_lenet(theta_row, x, y):
    """(loss64, g64 [P]): float64 torch autograd over the functional forward -- the yardstick of
    the GN-LeNet forward / backward probe and of tests/test_gpu_train_gnlenet.py."""
    return reference_gn_lenet(theta_row, x, y, torch.float64)


def probe_gn_lenet(model, x, y, params, device, sizes, flag=FLAG_GN, whose="the"):
    """The group count and the layer order cannot be read from parameter shapes: require that the
    gradient kernel agrees with model.forward + nll_loss + backward on the CPU on the samples x
    [B, Cin, H, W]: the loss within 1e-3 max(1, |loss|), every tensor's gradient within 1e-3 of
    that tensor's largest element (niidmix.evaluate's 1e-3 rule; another group count or layer order
    differs by O(0.1)).  Raises ValueError naming `flag`."""
    cin, h, w, c = sizes
    nb = int(x.shape[0])
    mdl = copy.deepcopy(model)
    for q in mdl.parameters():
        q.grad = None
    try:
        loss = F.nll_loss(mdl.forward(x, params), y)
        loss.backward()
    except Exception as e:                 # a forward that does not take these samples at all
        raise ValueError(f"{flag}: the model's forward failed on {whose} first {nb} samples "
                         f"({type(e).__name__}: {e})")
    g_cpu = [q.grad.reshape(-1) if q.grad is not None else torch.zeros(q.numel())
             for q in mdl.parameters()]
    dev = torch.device(device)
    p = ops.gnlenet_sizes(cin, h, w, c)[1]
    theta = torch.zeros((1, padded_ld(p)), dtype=torch.float32, device=dev)[:, :p]
    theta.copy_(_flat_params([mdl]))
    grad = torch.zeros((1, padded_ld(p)), dtype=torch.float32, device=dev)[:, :p]
    out = torch.empty(1, dtype=torch.float32, device=dev)
    bi = torch.arange(nb, dtype=torch.int32, device=dev).reshape(1, nb)
    bl = torch.tensor([nb], dtype=torch.int32, device=dev)
    ops.gnlenet_nll_grad_rows(theta, x.reshape(nb, -1).to(torch.float32).contiguous().to(dev),
                              y.to(torch.int32).to(dev), bi, bl,
                              torch.zeros(1, dtype=torch.int32, device=dev), grad, out, cin, h, w, c)
    got, loss = grad[0].cpu(), float(loss.detach())
    off = gn_lenet_offsets(cin, c, ops.gnlenet_sizes(cin, h, w, c)[0])
    worst = 0.0
    for i, gc in enumerate(g_cpu):
        d = float((got[off[i]:off[i + 1]] - gc).abs().max())
        ref = float(gc.abs().max())
        worst = max(worst, d / ref if ref > 0 else (0.0 if d == 0 else float("inf")))
        if d != d:
            worst = float("nan")
            break
    dl = abs(float(out[0]) - loss)
    if not worst <= 1e-3 or not dl <= 1e-3 * max(1.0, abs(loss)):
        raise ValueError(
            f"{flag}: the model's forward is not GN-LeNet's (5 x 5 convolutions of 32 / 32 / 64 "
            f"channels, GroupNorm(2), conv-pool-norm then conv-norm-pool twice, one Linear): on "
            f"{whose} first {nb} samples the kernel's loss {float(out[0]):.6g} / gradient differ from "
            f"forward + nll_loss + backward on the CPU (loss {loss:.6g}, worst gradient error "
            f"{worst:.3g} of a tensor's largest element, bound 1e-3)")


def cut_rows(n, need, budget):
    """Rows per call such that need(rows) <= budget: n when everything fits, else halved until it
    does (DeviceEvaluator._gn_cut's rule); None when one row does not fit."""
    if need(1) > budget:
        return None
    k = n
    while need(k) > budget:
        k = (k + 1) // 2
    return k


class DeviceTrainer:
    """Data, parameters, gradients (and momentum) of one node list in HBM, and the round above."""

    def __init__(self, nodes, topology, params, device):
        from . import d_sgd
        shape = check_eligible(nodes, params, topology)
        self.kind = "linear" if len(shape) == 2 else "gn-lenet"
        self.flag = FLAG_GN if gn_enabled(params) else FLAG
        self.scratch_budget = None       # bytes of scratch per GN-LeNet gradient call (None:
        self.last_calls = 0              # SCRATCH_FRACTION of the free HBM); calls of the last round
        self.sizes = None                # (Cin, H, W, C) of a GN-LeNet run, set by _materialise
        self._free_budget = None         # the default budget, measured before the first gradient call
        if self.kind == "linear":
            self.k, self.c = shape
            self.p = self.c * self.k + self.c
        else:
            self.gn_shape = shape
            self.c = shape[1]
            self.p = gn_lenet_offsets(*shape)[-1]
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
            if self.kind == "gn-lenet":
                sizes = sample_sizes(tuple(x.shape[1:]), self.gn_shape, self.flag,
                                     f"node {nd['rank']}'s train-set")
                if self.sizes not in (None, sizes):
                    raise ValueError(f"{self.flag}: node {nd['rank']}'s samples are "
                                     f"{tuple(x.shape[1:])}, earlier nodes' {self.sizes[:3]}")
                self.sizes = sizes
            x = x.reshape(len(items), -1)
            if self.kind == "linear" and x.shape[1] != self.k:
                raise ValueError(f"{self.flag}: node {nd['rank']}'s samples flatten to {x.shape[1]} "
                                 f"values, the model takes K = {self.k}")
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
        from ._lib import lib
        n_buf = self.n_buf
        need = n_buf * self.n * self.ld * 4 + xs.numel() * 4
        if self.kind == "linear":
            need += 4 * int(lib.niidmix_linear_nll_grad_rows_scratch_elems(self.n, self.b_max, self.c))
        else:                  # one row's scratch at least; _gn_cut sizes the calls every round
            need += self._gn_need(1)
        free, _ = torch.cuda.mem_get_info(self.device)
        if need > 0.8 * free:
            raise RuntimeError(f"{self.flag}: {need / 2**30:.1f} GiB of device buffers ({n_buf} slabs of "
                               f"[{self.n}, {self.p}], the train-sets, scratch) do not fit in "
                               f"{free / 2**30:.1f} GiB of free HBM")

    def _gn_need(self, rows):
        from ._lib import lib
        return int(lib.niidmix_gnlenet_nll_grad_rows_scratch_bytes(rows, self.b_max, *self.sizes))

    def _gn_cut(self):
        """Rows per call of the GN-LeNet gradient kernel: as many as keep its scratch within the
        budget (a row's bits do not depend on the cut)."""
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
        if self.kind == "linear":
            ops.linear_nll_grad_rows(x, self.data, self.labels, bi, bl, self.rows, self.grad,
                                     self.loss, self.k, self.c)
            self.last_calls = 1
            return
        cut = self._gn_cut()
        self.last_calls = 0
        for a in range(0, self.n, cut):
            b = min(self.n, a + cut)
            ops.gnlenet_nll_grad_rows(x, self.data, self.labels, bi[a:b], bl[a:b], self.rows[a:b],
                                      self.grad, self.loss[a:b], *self.sizes)
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
        """probe_forward / probe_gn_lenet on node 0's first samples."""
        ts = nodes[0]["train-set"]
        nb = min(PROBE_SAMPLES, len(ts), self.b_max)
        items = [ts[j] for j in range(nb)]
        x = torch.stack([torch.as_tensor(s[0]) for s in items])
        y = torch.as_tensor([int(s[1]) for s in items], dtype=torch.int64)
        if self.kind == "linear":
            probe_forward(self.models[0], x, y, params, self.device, self.flag, "node 0's")
        else:
            probe_gn_lenet(self.models[0], x, y, params, self.device, self.sizes, self.flag, "node 0's")

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
