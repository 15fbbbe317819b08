"""The model families of the device paths: what depends on WHICH model niidmix.train trains or
niidmix.evaluate evaluates, stated once.  LINEAR (setup/model/linear.py: one nn.Linear(K, C),
log_softmax) and GN_LENET (setup/model/gn_lenet.py) have the same methods; family_of(model) picks
one from the parameters' shapes.  A family knows its shape(model) -- (K, C) / (Cin, C, F), C is
shape[1] in both -- and P(shape); the kernels' limits as refusals (the constants are niidmix.ops',
which checks its arguments against the same ones); sizes(), the one sample check, giving the
kernel's size arguments (K, C) / (Cin, H, W, C); its gradient and evaluation op and their scratch
in bytes behind one signature; whether a call's row list may be cut; and the forward probes.
GN-LeNet's row layout is ops.gnlenet_shapes, one table: the expected shapes, the offsets, the row
splitter, P and F follow from it.  The float64 yardsticks of the probes and of the GPU tests live
here as well.
"""
import copy
import math

import torch
import torch.nn.functional as F

from . import ops
from ._lib import lib
from .model import flatten
from .ops import GN_MAX_CIN, GN_MAX_HW, GN_MIN_HW, MAX_B_SLICED, MAX_BC, MAX_C

PROBE_SAMPLES = 8


# shapes and the row layout
def _fp32_trainable(ps):
    return all(q.dtype == torch.float32 and q.requires_grad for q in ps)


def linear_shape(model):
    """(K, C) when the model's parameters are exactly a [C, K] weight then a [C] bias, else None."""
    ps = list(model.parameters())
    if len(ps) != 2 or ps[0].dim() != 2 or ps[1].dim() != 1 or ps[1].shape[0] != ps[0].shape[0]:
        return None
    if not _fp32_trainable(ps):
        return None
    return int(ps[0].shape[1]), int(ps[0].shape[0])


def gn_lenet_shape(model):
    """(Cin, C, F) when the model's parameters are exactly GN-LeNet's 14 tensors in registration
    order, fp32 and trainable, else None."""
    ps = list(model.parameters())
    if len(ps) != 14 or ps[0].dim() != 4 or ps[12].dim() != 2 or not _fp32_trainable(ps):
        return None
    cin, (c, f) = int(ps[0].shape[1]), (int(v) for v in ps[12].shape)
    last = ops.GN_CHANNELS[-1]         # F is that many channels of what the poolings leave
    if [tuple(q.shape) for q in ps] != ops.gnlenet_shapes(cin, c, f) or cin < 1 or f < last or f % last:
        return None
    return cin, c, f


def gn_lenet_offsets(cin, c, f):
    """Start of each of the 14 tensors in a flattened row, and P at the end (15 values)."""
    out = [0]
    for sh in ops.gnlenet_shapes(cin, c, f):
        out.append(out[-1] + math.prod(sh))
    return out


def split_gn_lenet(theta_row, cin, hw):
    """The 14 tensors (views) of a flattened GN-LeNet row for samples [cin, *hw]; C follows from
    the row's length."""
    f = ops.gnlenet_sizes(cin, hw[0], hw[1], 1)[0]
    p = int(theta_row.numel())
    c, rem = divmod(p - gn_lenet_offsets(cin, 0, f)[-1], f + 1)
    if c < 1 or rem:
        raise ValueError(f"a row of {p} values is no GN-LeNet for samples of [{cin}, {hw[0]}, {hw[1]}]")
    off = gn_lenet_offsets(cin, c, f)
    return [theta_row[off[i]:off[i + 1]].reshape(sh) for i, sh in enumerate(ops.gnlenet_shapes(cin, c, f))]


# the yardsticks
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


# what the probes share
def _one_row(model, x, y, p, device):
    """A probe's one-row, one-job setup: (theta [1, P] padded as the trainer pads its slabs and
    holding the model, the samples x flattened [B, *] fp32, the labels int32, a zero int32 [1]
    and the int32 [1] holding B), all on `device`."""
    from .train import padded_ld
    dev, nb = torch.device(device), int(x.shape[0])
    theta = torch.zeros((1, padded_ld(p)), dtype=torch.float32, device=dev)[:, :p]
    theta.copy_(flatten([model], "cpu"))
    return (theta, x.reshape(nb, -1).to(torch.float32).contiguous().to(dev), y.to(torch.int32).to(dev),
            torch.zeros(1, dtype=torch.int32, device=dev), torch.tensor([nb], dtype=torch.int32, device=dev))


def _cpu_grad(model, x, y, params):
    """(a copy of the model holding forward + nll_loss + backward's gradients on the CPU, loss)."""
    mdl = copy.deepcopy(model)
    for q in mdl.parameters():
        q.grad = None
    loss = F.nll_loss(mdl.forward(x, params), y)
    loss.backward()
    return mdl, loss.detach()


def _kernel_grad(fam, mdl, x, y, sizes, device):
    """(gradient [P] on the CPU, loss) of the family's gradient kernel on the batch x, y."""
    p, nb = fam.P(fam.shape(mdl)), int(x.shape[0])
    theta, data, labels, zero, bl = _one_row(mdl, x, y, p, device)
    dev = theta.device
    grad = torch.zeros((1, theta.stride(0)), dtype=torch.float32, device=dev)[:, :p]    # padded alike
    out = torch.empty(1, dtype=torch.float32, device=dev)
    bi = torch.arange(nb, dtype=torch.int32, device=dev).reshape(1, nb)
    fam.grad_rows(theta, data, labels, bi, bl, zero, grad, out, sizes)
    return grad[0].cpu(), float(out[0])


class _Linear:
    kind = "linear"
    cut = False          # the launcher's split depends on the row count: one call, never cut
    reads_resident = False   # as it was: evaluation does not look for a resident round's slab
    shape = staticmethod(linear_shape)

    def P(self, shape):
        return shape[1] * shape[0] + shape[1]

    def limits(self, shape, flag, batch=None, large=False):
        """ValueError naming `flag` when the kernels do not hold C classes (or, for training,
        batches of `batch` samples).  `large` (--device-training-large-batch): batches beyond
        MAX_BC go to the sliced kernels, which hold MAX_B_SLICED samples."""
        c = shape[1]
        if large and batch is not None and c <= MAX_C:
            if batch > MAX_B_SLICED:
                raise ValueError(f"{flag}: batch-size = {batch} exceeds the sliced kernel's limit "
                                 f"(batch-size <= {MAX_B_SLICED})")
            return
        if batch is not None and (c > MAX_C or batch * c > MAX_BC):
            raise ValueError(f"{flag}: C = {c}, batch-size * C = {batch * c} exceed the kernel's limits "
                             f"(C <= {MAX_C}, batch-size * C <= {MAX_BC})")
        if c > MAX_C:
            raise ValueError(f"{flag}: C = {c} exceeds the kernel's limit (C <= {MAX_C})")

    def sizes(self, sh, shape, flag, what):
        """(K, C) for samples of shape `sh`; ValueError naming `flag` when they do not flatten to
        the model's K."""
        if math.prod(sh) != shape[0]:
            raise ValueError(f"{flag}: the samples of {what} flatten to {math.prod(sh)} values, the "
                             f"model takes K = {shape[0]}")
        return shape

    @staticmethod
    def sliced(b_max, sizes, large):
        """Under --device-training-large-batch (`large`) a call goes to the sliced op exactly when
        the existing kernel does not take its shape."""
        return bool(large) and b_max * sizes[1] > MAX_BC

    def grad_rows(self, theta, data, labels, bi, bl, rows, grad, loss, sizes, large=False):
        op = ops.linear_nll_grad_rows_sliced if self.sliced(bi.shape[1], sizes, large) else \
            ops.linear_nll_grad_rows
        op(theta, data, labels, bi, bl, rows, grad, loss, *sizes)

    def eval_rows(self, theta, data, labels, rows, start, length, max_len, loss_sum, correct, sizes):
        ops.linear_eval_rows(theta, data, labels, rows, start, length, max_len, loss_sum, correct,
                             None, *sizes)

    def grad_scratch_bytes(self, rows, b_max, sizes, large=False):
        if self.sliced(b_max, sizes, large):
            return 4 * int(lib.niidmix_linear_nll_grad_rows_sliced_scratch_elems(rows, b_max, *sizes))
        return 4 * int(lib.niidmix_linear_nll_grad_rows_scratch_elems(rows, b_max, sizes[1]))  # fp32 elements

    def eval_scratch_bytes(self, jobs, max_len, sizes):
        return int(lib.niidmix_linear_eval_rows_scratch_bytes(jobs, max_len, sizes[1]))

    def probe_grad(self, model, x, y, params, device, sizes, flag, whose="the"):
        """Require that model.forward + nll_loss + backward on the CPU agree with the gradient
        kernel on the samples x (as the model takes them) with labels y, under the tests' tolerance
        (both are within 1e-5 A of the float64 result, hence within 2e-5 A of each other).  Raises
        ValueError naming `flag`."""
        nb = int(x.shape[0])
        mdl, loss = _cpu_grad(model, x, y, params)
        g_cpu = torch.cat([q.grad.reshape(-1) for q in mdl.parameters()])
        got, out = _kernel_grad(self, mdl, x, y, sizes, device)
        w, b = [q.detach() for q in mdl.parameters()]
        l64, _, a = fp64_reference(w, b, x.reshape(nb, -1).to(torch.float32), y)
        dg = (got.double() - g_cpu.double()).abs()
        dl = abs(out - float(loss))
        if not bool((dg <= 2e-5 * a).all()) or not dl <= 2e-5 * max(abs(float(l64)), 1.0):
            raise ValueError(
                f"{flag}: the model's forward is not log_softmax(Linear(x.view(-1, K))): on {whose} "
                f"first {nb} samples the kernel's loss {out:.6g} / gradient differ from "
                f"forward + nll_loss + backward on the CPU (loss {float(loss):.6g}, worst gradient "
                f"ratio {float((dg / a.clamp_min(1e-300)).max()):.3g} of the bound)")

    probe_eval = probe_grad      # the evaluation kernel computes the gradient kernel's forward


class _GNLeNet:
    kind = "gn-lenet"
    cut = True           # a row's bits do not depend on the cut
    reads_resident = True    # evaluation reads a fresh resident round's output slab in place
    shape = staticmethod(gn_lenet_shape)

    def P(self, shape):
        return gn_lenet_offsets(*shape)[-1]

    def limits(self, shape, flag, batch=None, large=False):
        """ValueError naming `flag` when the kernels do not hold C classes or Cin channels."""
        cin, c, _ = shape
        if c > MAX_C:
            raise ValueError(f"{flag}: C = {c} exceeds the kernel's limit (C <= {MAX_C})")
        if cin > GN_MAX_CIN:
            raise ValueError(f"{flag}: {cin} input channels exceed the kernel's limit "
                             f"(Cin <= {GN_MAX_CIN})")

    def sizes(self, sh, shape, flag, what):
        """(Cin, H, W, C) for samples of shape `sh`; ValueError naming `flag` when they are not
        [Cin, H, W] images the kernels take, giving the classifier's F."""
        cin, c, f = shape
        sh = None if sh is None else tuple(sh)
        if sh is None or len(sh) != 3 or sh[0] != cin:
            raise ValueError(f"{flag}: the samples of {what} have shape {sh}, GN-LeNet takes "
                             f"[{cin}, H, W]")
        h, w = int(sh[1]), int(sh[2])
        if not (GN_MIN_HW <= h <= GN_MAX_HW and GN_MIN_HW <= w <= GN_MAX_HW):
            raise ValueError(f"{flag}: samples of {h} x {w} in {what}: the kernel takes "
                             f"{GN_MIN_HW} <= H, W <= {GN_MAX_HW}")
        got = ops.gnlenet_sizes(cin, h, w, c)[0]
        if got != f:
            raise ValueError(f"{flag}: samples of shape {sh} in {what} give GN-LeNet {got} "
                             f"features, the model's classifier takes F = {f}")
        return cin, h, w, c

    def grad_rows(self, theta, data, labels, bi, bl, rows, grad, loss, sizes, large=False):
        ops.gnlenet_nll_grad_rows(theta, data, labels, bi, bl, rows, grad, loss, *sizes)

    def eval_rows(self, theta, data, labels, rows, start, length, max_len, loss_sum, correct, sizes):
        ops.gnlenet_eval_rows(theta, data, labels, rows, start, length, max_len, loss_sum, correct,
                              None, None, *sizes)

    def grad_scratch_bytes(self, rows, b_max, sizes, large=False):
        return int(lib.niidmix_gnlenet_nll_grad_rows_scratch_bytes(rows, b_max, *sizes))

    def eval_scratch_bytes(self, jobs, max_len, sizes):
        return int(lib.niidmix_gnlenet_eval_rows_scratch_bytes(jobs, max_len, *sizes))

    _NOT_GN_LENET = ("the model's forward is not GN-LeNet's (5 x 5 convolutions of 32 / 32 / 64 "
                     "channels, GroupNorm(2), conv-pool-norm then conv-norm-pool twice, one Linear)")

    def probe_grad(self, model, x, y, params, device, sizes, flag, whose="the"):
        """The group count and the layer order cannot be read from parameter shapes: require that
        the gradient kernel agrees with model.forward + nll_loss + backward on the CPU on the
        samples x [B, Cin, H, W]: the loss within 1e-3 max(1, |loss|), every tensor's gradient
        within 1e-3 of that tensor's largest element (probe_eval's 1e-3 rule; another group count
        or layer order differs by O(0.1)).  Raises ValueError naming `flag`."""
        nb = int(x.shape[0])
        try:
            mdl, loss = _cpu_grad(model, x, y, params)
        except Exception as e:                 # a forward that does not take these samples at all
            raise ValueError(f"{flag}: the model's forward failed on {whose} first {nb} samples "
                             f"({type(e).__name__}: {e})")
        g_cpu = [q.grad.reshape(-1) if q.grad is not None else torch.zeros(q.numel())
                 for q in mdl.parameters()]
        got, out = _kernel_grad(self, mdl, x, y, sizes, device)
        loss = float(loss)
        off = gn_lenet_offsets(*self.shape(mdl))
        worst = 0.0
        for i, gc in enumerate(g_cpu):
            d = float((got[off[i]:off[i + 1]] - gc).abs().max())
            ref = float(gc.abs().max())
            worst = max(worst, d / ref if ref > 0 else (0.0 if d == 0 else float("inf")))
            if d != d:
                worst = float("nan")
                break
        dl = abs(out - loss)
        if not worst <= 1e-3 or not dl <= 1e-3 * max(1.0, abs(loss)):
            raise ValueError(
                f"{flag}: {self._NOT_GN_LENET}: on "
                f"{whose} first {nb} samples the kernel's loss {out:.6g} / gradient differ from "
                f"forward + nll_loss + backward on the CPU (loss {loss:.6g}, worst gradient error "
                f"{worst:.3g} of a tensor's largest element, bound 1e-3)")

    def probe_eval(self, model, x, y, params, device, sizes, flag):
        """The same for the evaluation kernel: require that its log-softmaxed logits on the
        samples x agree with model.forward on the CPU within 1e-3 max(1, max |z|) (another
        architecture differs by O(0.1))."""
        from . import d_sgd
        d_sgd.synchronize()
        nb, c = int(x.shape[0]), sizes[3]
        with torch.no_grad():
            want = model.forward(x, params).detach().to(torch.float32)
        theta, data, labels, zero, bl = _one_row(model, x, y, self.P(self.shape(model)), device)
        dev = theta.device
        z = torch.zeros((1, nb, c), dtype=torch.float32, device=dev)
        ops.gnlenet_eval_rows(theta, data, labels, zero, zero, bl, nb,
                              torch.empty(1, dtype=torch.float64, device=dev),
                              torch.empty(1, dtype=torch.int32, device=dev), None, z, *sizes)
        z = z[0].cpu()
        got = torch.log_softmax(z, 1)
        bound = 1e-3 * max(1.0, float(z.abs().max()))
        worst = float((got - want).abs().max()) if tuple(want.shape) == tuple(got.shape) else float("nan")
        if not worst <= bound:
            raise ValueError(
                f"{flag}: {self._NOT_GN_LENET}: on "
                f"the first {nb} samples the kernel's log-probabilities differ from forward on the "
                f"CPU by {worst:.3g} (bound {bound:.3g})")


LINEAR, GN_LENET = _Linear(), _GNLeNet()


def family_of(model):
    """(family, shape) of a model the device paths take, else None."""
    for fam in (LINEAR, GN_LENET):
        shape = fam.shape(model)
        if shape is not None:
            return fam, shape
    return None
