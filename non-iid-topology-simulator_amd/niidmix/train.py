"""Local training on the device for linear models (`--device-training`).

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
"""
import copy
import os

import torch
import torch.nn.functional as F

from . import ops
from .topology import to_csr

FLAG = "--device-training"
PROBE_SAMPLES = 8
# the kernel's limits (include/niidmix.h)
MAX_C = 1024
MAX_BC = 32768


def enabled(params):
    return bool(params.get("algorithm", {}).get("device-training"))


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
            raise ValueError(f"{FLAG}: node {node['rank']}'s train-iterator yields samples, not "
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


def check_eligible(nodes, params):
    """The refusals that need no GPU (d_sgd.init calls this): raises ValueError naming the flag."""
    from . import d_sgd
    alg = params["algorithm"]
    if params["topology"]["name"] == "sample":
        raise ValueError(f"{FLAG} does not support the 'sample' topology")
    if alg.get("clique-gradient") or alg.get("unbiased-gradient"):
        raise ValueError(f"{FLAG} does not support --clique-gradient / --unbiased-gradient")
    env = os.environ.get("NIIDMIX_DEVICES")
    if env and len([i for i in env.split(",") if i.strip()]) > 1:
        raise ValueError(f"{FLAG} runs on one device; NIIDMIX_DEVICES lists several")
    if not nodes:
        raise ValueError(f"{FLAG}: no nodes")
    shape = linear_shape(nodes[0]["model"])
    lr, mom = float(alg["learning-rate"]), d_sgd._momentum(params)
    for nd in nodes:
        if shape is None or linear_shape(nd["model"]) != shape:
            raise ValueError(f"{FLAG} needs models whose parameters are exactly a [C, K] weight and "
                             f"a [C] bias, the same on every node (node {nd['rank']} differs)")
        opt = nd.get("optimizer")
        ps = list(nd["model"].parameters())
        if not d_sgd._plugin_sgd(opt, lr, mom) or len(opt.param_groups[0]["params"]) != 2 or \
                any(a is not b for a, b in zip(opt.param_groups[0]["params"], ps)):
            raise ValueError(f"{FLAG} needs the plugin's SGD optimizer (niidmix.d_sgd.optimizer) at "
                             f"the run's learning rate and momentum (node {nd['rank']})")
    k, c = shape
    b = int(alg["batch-size"])
    if c > MAX_C or b * c > MAX_BC:
        raise ValueError(f"{FLAG}: C = {c}, batch-size * C = {b * c} exceed the kernel's limits "
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


class DeviceTrainer:
    """Data, parameters, gradients (and momentum) of one node list in HBM, and the round above."""

    def __init__(self, nodes, topology, params, device):
        from . import d_sgd
        self.k, self.c = check_eligible(nodes, params)
        self.p = self.c * self.k + self.c
        self.ld = padded_ld(self.p)
        self.n = len(nodes)
        self.device = torch.device(device)
        self.models = [nd["model"] for nd in nodes]
        self.b_max = int(params["algorithm"]["batch-size"])
        self.lr = float(params["algorithm"]["learning-rate"])
        self.momentum = d_sgd._momentum(params)
        if self.momentum != 0.0 and d_sgd._momentum_state(nodes) != "none":
            raise ValueError(f"{FLAG} was switched on while the CPU optimizers hold momentum "
                             "buffers: handing them to the device mid-run is not supported")
        xs, ys, self.offsets = self._materialise(nodes)
        self._check_fit(xs)
        dev = self.device
        self.data = xs.to(dev)
        self.labels = ys.to(dev)
        n_buf = 3 + (self.momentum != 0.0)
        slabs = [torch.zeros((self.n, self.ld), dtype=torch.float32, device=dev) for _ in range(n_buf)]
        self.theta = [s[:, :self.p] for s in slabs[:2]]      # ping-pong: mixing is out-of-place
        self.grad = slabs[2][:, :self.p]
        self.mbuf = slabs[3][:, :self.p] if self.momentum != 0.0 else None
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
                raise ValueError(f"{FLAG}: node {nd['rank']} has an empty train-set")
            x = torch.stack([torch.as_tensor(s[0]) for s in items]).reshape(len(items), -1)
            if x.shape[1] != self.k:
                raise ValueError(f"{FLAG}: node {nd['rank']}'s samples flatten to {x.shape[1]} "
                                 f"values, the model takes K = {self.k}")
            y = torch.as_tensor([int(s[1]) for s in items], dtype=torch.int64)
            if int(y.min()) < 0 or int(y.max()) >= self.c:
                raise ValueError(f"{FLAG}: node {nd['rank']} has a label outside [0, {self.c})")
            xs.append(x.to(torch.float32))
            ys.append(y.to(torch.int32))
            offsets.append(offsets[-1] + len(items))
        if offsets[-1] >= 2 ** 31:
            raise ValueError(f"{FLAG}: {offsets[-1]} samples exceed int32 indices")
        return torch.cat(xs).contiguous(), torch.cat(ys).contiguous(), offsets

    def _check_fit(self, xs):
        """ResidentRound.fits-style arithmetic: slabs, data and the kernel's scratch against the
        free HBM.  No fit is an error: there is no silent CPU fallback under an explicit flag."""
        from ._lib import lib
        n_buf = 3 + (self.momentum != 0.0)
        need = n_buf * self.n * self.ld * 4 + xs.numel() * 4 + \
            4 * int(lib.niidmix_linear_nll_grad_rows_scratch_elems(self.n, self.b_max, self.c))
        free, _ = torch.cuda.mem_get_info(self.device)
        if need > 0.8 * free:
            raise RuntimeError(f"{FLAG}: {need / 2**30:.1f} GiB of device buffers ({n_buf} slabs of "
                               f"[{self.n}, {self.p}], the train-sets, scratch) do not fit in "
                               f"{free / 2**30:.1f} GiB of free HBM")

    def _probe(self, nodes, params):
        """probe_forward on node 0's first samples."""
        ts = nodes[0]["train-set"]
        nb = min(PROBE_SAMPLES, len(ts), self.b_max)
        items = [ts[j] for j in range(nb)]
        x = torch.stack([torch.as_tensor(s[0]) for s in items])
        y = torch.as_tensor([int(s[1]) for s in items], dtype=torch.int64)
        probe_forward(self.models[0], x, y, params, self.device, FLAG, "node 0's")

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
        torch.cuda.synchronize(self.device)      # nothing reads the old descriptors any more
        self.mixer = ops.Mixer(csr=csr, cliques=topology.get("cliques"), device=self.device)
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
                raise ValueError(f"{FLAG}: node {nodes[i]['rank']} drew a batch its train-set or "
                                 "the batch size does not allow")
            bi[i, :k] = idx.numpy() + self.offsets[i]
            bl[i] = k
        self.idx_dev.copy_(self.idx_host, non_blocking=True)           # one H2D copy
        x, y = self.theta[self.cur], self.theta[1 - self.cur]
        ops.linear_nll_grad_rows(x, self.data, self.labels, self.idx_dev[:nb].view(self.n, self.b_max),
                                 self.idx_dev[nb:], self.rows, self.grad, self.loss, self.k, self.c)
        if self.momentum != 0.0:
            ops.sgd_momentum_step_rows(x, self.grad, self.mbuf, self.rows, -self.lr, self.momentum,
                                       self.mom_steps == 0)
            self.mom_steps += 1
        else:
            ops.sgd_step_rows(x, self.grad, self.rows, -self.lr)
        self.mixer(x, out=y, mode=mode)
        self.cur = 1 - self.cur
        loss = self.loss.cpu().tolist()
        self.write_back()
        return {nd["rank"]: float(v) for nd, v in zip(nodes, loss)}, epoch_done
