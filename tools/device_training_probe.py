#!/usr/bin/env python
"""Device-training probe (measurement tool): what niidmix_linear_nll_grad_rows_f32 and the
--device-training round cost on one GPU, at the two shapes
    ref   N 1000, K 784,  C 10,   B 125   (the reference's linear model on MNIST)
    e2e   N 1000, K 1023, C 1024, B 16    (P = 2^20, the E2E shape of DESIGN §5)

  kernel   device-event times of single launches of the gradient call, alternating with
           niidmix_stream_copy_f32 over the parameter slab within every repetition, reported
           against the algorithmic bytes 4 (2 N P + sum(len) K) as a share of 8 TB/s and of the
           stream copy's rate in the same run.
  rounds   d_sgd.next_step on the headline topology (d-cliques 1000, cliques of 100,
           fully-connected), flag off and flag on interleaved round by round after a warm-up:
           median, minimum and maximum of each.

    python tools/device_training_probe.py kernel --shape ref [--warmup 5] [--reps 20]
    python tools/device_training_probe.py rounds --shape ref [--warmup 2] [--rounds 10]
    python tools/device_training_probe.py all        # every step as a child process of its own

GN-LeNet (niidmix_gnlenet_nll_grad_rows_f32, --device-training-gn-lenet), at the two shapes
    gn-cifar   N 1000, 3 x 32 x 32, C 10, B 20     gn-mnist   N 100, 1 x 28 x 28, C 10, B 128
  gn-kernel  the gradient call against three yardsticks, all four alternating within every
             repetition: the CPU loop (forward + nll_loss + backward of the module, torch's
             threads as set, on a few nodes, scaled to N), torch autograd on the device (the
             same module, looped over a few nodes, scaled to N), and niidmix_stream_copy_f32 over
             the bytes the call must read (parameters and batch samples).  Device candidates by
             device events, the CPU loop by the host clock.
  gn-rounds  as `rounds`, for GN-LeNet models and the --device-training-gn-lenet flag.

    python tools/device_training_probe.py gn-kernel --shape gn-cifar [--warmup 5] [--reps 20]
    python tools/device_training_probe.py gn-rounds --shape gn-mnist [--warmup 2] [--rounds 10]

Gradient averaging (--clique-gradient under --device-training):
  fused-step  niidmix_grad_segment_mean_sgd_step_f32 against its two-launch composition
              (niidmix_grad_segment_mean_f32, then niidmix_sgd_step_rows_f32 or
              niidmix_sgd_momentum_step_rows_f32) on 1000 rows in 10 cliques of 100, at P = 2^20
              (--shape e2e) or GN-LeNet's P for 3 x 32 x 32, C = 10 (--shape gn-cifar), momentum 0
              and 0.9 (a later step: buf is read), all four alternating within every repetition;
              device events; each against its algorithmic bytes as a share of 8 TB/s, and the
              measured time ratio next to the ratio of the byte counts.  The two results are
              compared bit for bit at the end.
  rounds / gn-rounds take --clique-gradient and --momentum M: both paths then average the
              cliques' gradients.

    python tools/device_training_probe.py fused-step --shape e2e [--warmup 5] [--reps 20]
    python tools/device_training_probe.py gn-rounds --shape gn-cifar --clique-gradient --momentum 0.9

Long batches (niidmix_linear_nll_grad_rows_sliced_f32, --device-training-large-batch):
  large-batch  the sliced call at (rows, B) = (1, 12 800), (10, 6000), (100, 3277) with K 784, C 10,
               against the bytes it must move as a share of 8 TB/s, its four kernels apart at the
               first shape (torch's profiler); the sliced and the existing entry alternating at
               (1, 3276) and (1000, 3276), the largest batch both take; and the centralised round:
               d_sgd.next_step at one node, 60 000 x 784 synthetic samples, batch 12 800, under the
               flag with --device-sampling --device-sampling-cached against the same round with
               every device flag off, alternating round by round.  Device events for the calls, the
               host clock around next_step + synchronize for the rounds.

    python tools/device_training_probe.py large-batch [--warmup 5] [--reps 20]

`all` runs the four steps one after the other, each in a fresh process under its own time limit,
and stops at the first that fails.  Every step prints one JSON line.
"""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "non-iid-topology-simulator_amd")]

SHAPES = {"ref": (1000, 784, 10, 125), "e2e": (1000, 1023, 1024, 16)}
GN_SHAPES = {"gn-cifar": (1000, 3, 32, 32, 10, 20), "gn-mnist": (100, 1, 28, 28, 10, 128)}
STEP_LIMIT_S = {"kernel": 180, "rounds": 420}


def _gn_lenet(cin, h, w, c):
    """A module with GN-LeNet's 14 parameter tensors and forward (setup/model/gn_lenet.py's
    layers), built here so that the tool needs no dataset code."""
    import torch
    import torch.nn.functional as F
    from niidmix import ops

    class GNLeNet(torch.nn.Module):
        def __init__(self):
            super().__init__()
            gn = torch.nn.GroupNorm
            self.features = torch.nn.Sequential(
                torch.nn.Conv2d(cin, 32, 5, padding=2), torch.nn.MaxPool2d(3, 2), gn(2, 32),
                torch.nn.ReLU(),
                torch.nn.Conv2d(32, 32, 5, padding=2), gn(2, 32), torch.nn.MaxPool2d(3, 2),
                torch.nn.ReLU(),
                torch.nn.Conv2d(32, 64, 5, padding=2), gn(2, 64), torch.nn.MaxPool2d(3, 2),
                torch.nn.ReLU())
            self.classifier = torch.nn.Sequential(torch.nn.Linear(ops.gnlenet_sizes(cin, h, w, c)[0], c))

        def forward(self, x, params):
            return F.log_softmax(self.classifier(torch.flatten(self.features(x), 1)), dim=1)

    return GNLeNet


def gn_kernel(a):
    import copy
    import torch
    import torch.nn.functional as F
    from niidmix import _lib, ops, train
    n, cin, h, w, c, b = GN_SHAPES[a.shape]
    n = a.nodes or n
    dev = torch.device("cuda:0")
    k = cin * h * w
    p = ops.gnlenet_sizes(cin, h, w, c)[1]
    ld = train.padded_ld(p)
    torch.manual_seed(3)
    mdl = _gn_lenet(cin, h, w, c)()
    row = torch.cat([q.detach().reshape(-1) for q in mdl.parameters()])
    gen = torch.Generator(device=dev).manual_seed(1)
    s = n * 2 * b
    theta = torch.zeros(n, ld, device=dev)
    theta[:, :p] = row.to(dev) * (1 + 0.01 * torch.randn(n, p, device=dev, generator=gen))
    grad = torch.zeros(n, ld, device=dev)
    data = torch.randn(s, k, device=dev, generator=gen)
    labels = torch.randint(0, c, (s,), device=dev, generator=gen).to(torch.int32)
    idx = torch.stack([torch.randperm(2 * b, device=dev, generator=gen)[:b] + 2 * b * i
                       for i in range(n)]).to(torch.int32).contiguous()
    blen = torch.full((n,), b, dtype=torch.int32, device=dev)
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    loss = torch.empty(n, device=dev)
    lib = _lib.lib
    nbytes = int(lib.niidmix_gnlenet_nll_grad_rows_scratch_bytes(n, b, cin, h, w, c))
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    strm = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    read = n * p + n * b * k                           # floats the call must read
    src, dst = torch.empty(read - read % 4, device=dev), torch.empty(read - read % 4, device=dev)

    def grad_call():
        _lib.check(lib.niidmix_gnlenet_nll_grad_rows_f32(
            theta.data_ptr(), ld, data.data_ptr(), labels.data_ptr(), idx.data_ptr(), blen.data_ptr(),
            b, rows.data_ptr(), n, grad.data_ptr(), ld, loss.data_ptr(), cin, h, w, c,
            scratch.data_ptr(), nbytes, strm), "grad")

    def copy_call():
        _lib.check(lib.niidmix_stream_copy_f32(src.data_ptr(), dst.data_ptr(), src.numel(), strm), "copy")

    def loop(model, x, y, nodes):
        for i in range(nodes):                         # one node's CPU-path step, minus the optimizer
            model.zero_grad(set_to_none=True)
            F.nll_loss(model.forward(x[i], None), y[i]).backward()

    n_dev, n_cpu = min(n, a.loop_nodes_device), min(n, a.loop_nodes_cpu)
    xb = data[idx[:n_dev].long()].reshape(n_dev, b, cin, h, w)
    yb = labels[idx[:n_dev].long()].long()
    mdl_dev = copy.deepcopy(mdl).to(dev)
    xc, yc = xb[:n_cpu].cpu(), yb[:n_cpu].cpu()
    cands = [("copy", copy_call, 1.0, True), ("grad", grad_call, 1.0, True),
             ("device_autograd", lambda: loop(mdl_dev, xb, yb, n_dev), n / n_dev, True),
             ("cpu_loop", lambda: loop(mdl, xc, yc, n_cpu), n / n_cpu, False)]
    times = {name: [] for name, _, _, _ in cands}
    for rep_i in range(a.warmup + a.reps):
        for name, fn, scale, on_dev in cands:
            torch.cuda.synchronize(dev)
            s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            s0.record()
            fn()
            e0.record()
            e0.synchronize()
            dt = s0.elapsed_time(e0) * 1e-3 if on_dev else time.perf_counter() - t0
            if rep_i >= a.warmup:
                times[name].append(dt * scale)
    assert bool(torch.isfinite(loss).all())
    out = {"step": "gn-kernel", "shape": a.shape, "n": n, "sample": [cin, h, w], "c": c, "b": b,
           "warmup": a.warmup, "reps": a.reps, "threads": torch.get_num_threads(),
           "loop_nodes_device": n_dev, "loop_nodes_cpu": n_cpu, "scratch_bytes": nbytes,
           "read_bytes": 4 * read, "device": torch.cuda.get_device_name(dev),
           "lib_sha16": _lib.lib_sha16()}
    for name, _, _, _ in cands:
        t = times[name]
        out[name] = {"median_ms": statistics.median(t) * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3}
    for name in ("copy", "device_autograd", "cpu_loop"):
        out["grad_over_" + name] = out["grad"]["median_ms"] / out[name]["median_ms"]
    print(json.dumps(out))


def kernel(a):
    import torch
    from niidmix import _lib, train
    n, k, c, b = SHAPES[a.shape]
    n = a.nodes or n
    dev = torch.device("cuda:0")
    p = c * k + c
    ld = train.padded_ld(p)
    gen = torch.Generator(device=dev).manual_seed(1)
    s = n * 2 * b
    theta = (torch.rand(n, ld, device=dev, generator=gen) - 0.5) * (2 / k ** 0.5)
    grad = torch.zeros(n, ld, device=dev)
    data = torch.rand(s, k, device=dev, generator=gen)
    labels = torch.randint(0, c, (s,), device=dev, generator=gen).to(torch.int32)
    idx = torch.stack([torch.randperm(2 * b, device=dev, generator=gen)[:b] + 2 * b * i
                       for i in range(n)]).to(torch.int32).contiguous()
    blen = torch.full((n,), b, dtype=torch.int32, device=dev)
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    loss = torch.empty(n, device=dev)
    lib = _lib.lib
    elems = int(lib.niidmix_linear_nll_grad_rows_scratch_elems(n, b, c))
    scratch = torch.empty(elems, device=dev)
    strm = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    numel = n * ld - (n * ld) % 4

    def grad_call():
        return lib.niidmix_linear_nll_grad_rows_f32(
            theta.data_ptr(), ld, data.data_ptr(), labels.data_ptr(), idx.data_ptr(), blen.data_ptr(),
            b, rows.data_ptr(), n, grad.data_ptr(), ld, loss.data_ptr(), k, c, scratch.data_ptr(),
            elems, strm)

    def copy_call():
        return lib.niidmix_stream_copy_f32(theta.data_ptr(), grad.data_ptr(), numel, strm)

    calls = [("copy", copy_call, 8 * numel), ("grad", grad_call, 4 * (2 * n * p + n * b * k))]
    times = {name: [] for name, _, _ in calls}
    for rep in range(a.warmup + a.reps):
        for name, fn, _ in calls:
            s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            _lib.check(fn(), name)
            e0.record()
            e0.synchronize()
            if rep >= a.warmup:
                times[name].append(s0.elapsed_time(e0) * 1e-3)
    assert bool(torch.isfinite(loss).all())
    out = {"step": "kernel", "shape": a.shape, "n": n, "k": k, "c": c, "b": b, "warmup": a.warmup,
           "reps": a.reps, "device": torch.cuda.get_device_name(dev), "lib_sha16": _lib.lib_sha16()}
    for name, _, nbytes in calls:
        t = times[name]
        med = statistics.median(t)
        out[name] = {"bytes": nbytes, "median_ms": med * 1e3, "min_ms": min(t) * 1e3,
                     "max_ms": max(t) * 1e3, "gbps_median": nbytes / med / 1e9}
    out["grad"]["share_of_8TBps"] = out["grad"]["gbps_median"] / 8000
    out["grad"]["share_of_stream_copy"] = out["grad"]["gbps_median"] / out["copy"]["gbps_median"]
    print(json.dumps(out))


def fused_step(a):
    import torch
    from niidmix import _lib, ops, train
    n = a.nodes or 1000
    p = ops.gnlenet_sizes(3, 32, 32, 10)[1] if a.shape == "gn-cifar" else 1 << 20
    ld = train.padded_ld(p)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    size = min(100, n)
    cliques = [list(range(s0, min(s0 + size, n))) for s0 in range(0, n, size)]
    seg_ptr = torch.tensor([0] + [c[-1] + 1 for c in cliques], dtype=torch.int32, device=dev)
    rows = torch.arange(n, dtype=torch.int32, device=dev)                  # seg_row and the step's rows
    g = torch.randn(n, ld, device=dev, generator=gen)
    p0 = torch.randn(n, ld, device=dev, generator=gen)
    b0 = torch.randn(n, ld, device=dev, generator=gen)
    slabs = {k: torch.empty(n, ld, device=dev) for k in ("p_f", "b_f", "p_c", "b_c", "avg")}
    lib = _lib.lib
    strm = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = {k: v.data_ptr() for k, v in slabs.items()}
    n_seg, lr = len(cliques), -0.05

    def fused(m):
        return lib.niidmix_grad_segment_mean_sgd_step_f32(
            ptr["p_f"], ld, g.data_ptr(), ld, ptr["b_f"] if m else None, ld if m else 0, p, n_seg,
            seg_ptr.data_ptr(), rows.data_ptr(), n, lr, m, 0, strm)

    def parts(m):
        rc = lib.niidmix_grad_segment_mean_f32(g.data_ptr(), ld, ptr["avg"], ld, n, p, n_seg,
                                               seg_ptr.data_ptr(), rows.data_ptr(), strm)
        if rc:
            return rc
        if m:
            return lib.niidmix_sgd_momentum_step_rows_f32(ptr["p_c"], ld, ptr["avg"], ld, ptr["b_c"], ld,
                                                          p, rows.data_ptr(), n, lr, m, 0, strm)
        return lib.niidmix_sgd_step_rows_f32(ptr["p_c"], ld, ptr["avg"], ld, p, rows.data_ptr(), n, lr, strm)

    # bytes per node-parameter: include/niidmix.h, niidmix_grad_segment_mean_sgd_step_f32
    cands = [("fused_m0", fused, 0.0, 12), ("parts_m0", parts, 0.0, 20),
             ("fused_m09", fused, 0.9, 20), ("parts_m09", parts, 0.9, 28)]
    times = {name: [] for name, _, _, _ in cands}
    for k, v in slabs.items():
        v.copy_(b0 if k.startswith("b_") else p0)
    for r in range(a.warmup + a.reps):
        for name, fn, m, _ in cands:
            s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            _lib.check(fn(m), name)
            e0.record()
            e0.synchronize()
            if r >= a.warmup:
                times[name].append(s0.elapsed_time(e0) * 1e-3)
    same = {}
    for m in (0.0, 0.9):                       # the timed calls ran on drifting values: compare afresh
        for k in ("p_f", "p_c"):
            slabs[k].copy_(p0)
        for k in ("b_f", "b_c"):
            slabs[k].copy_(b0)
        _lib.check(fused(m), "fused")
        _lib.check(parts(m), "parts")
        torch.cuda.synchronize(dev)
        same[str(m)] = bool(torch.equal(slabs["p_f"].view(torch.int32), slabs["p_c"].view(torch.int32)) and
                            torch.equal(slabs["b_f"].view(torch.int32), slabs["b_c"].view(torch.int32)))
    out = {"step": "fused-step", "shape": a.shape, "n": n, "p": p, "cliques": n_seg, "warmup": a.warmup,
           "reps": a.reps, "device": torch.cuda.get_device_name(dev), "lib_sha16": _lib.lib_sha16(),
           "bitwise_equal": same}
    for name, _, _, bpe in cands:
        t = times[name]
        med = statistics.median(t)
        out[name] = {"bytes": bpe * n * p, "median_ms": med * 1e3, "min_ms": min(t) * 1e3,
                     "max_ms": max(t) * 1e3, "share_of_8TBps": bpe * n * p / med / 8e12}
    for tag, pred in (("m0", 12 / 20), ("m09", 20 / 28)):
        out["ratio_" + tag] = {"measured": out["fused_" + tag]["median_ms"] / out["parts_" + tag]["median_ms"],
                               "predicted_from_bytes": pred}
    print(json.dumps(out))
    if not all(same.values()):
        sys.exit("device_training_probe: the fused kernel and the two launches differ")


def rounds(a):
    import torch
    import torch.nn.functional as F
    from niidmix import d_sgd
    from niidmix.generate import dcliques
    from niidmix.topology import mh_csr
    gn = a.shape in GN_SHAPES
    if gn:
        n, cin, h, w, c, b = GN_SHAPES[a.shape]
        k = cin * h * w
    else:
        n, k, c, b = SHAPES[a.shape]
    n = a.nodes or n
    per_node = 2 * b

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = torch.nn.Linear(k, c)

        def forward(self, x, params):
            return F.log_softmax(self.fc(x.view(-1, k)), dim=1)

    edges, cliques = dcliques(n, min(100, n), "fully-connected", 1337)
    topo = {"edges": edges, "csr": mh_csr(n, edges), "weights": torch.tensor([]), "cliques": cliques}
    g = torch.Generator().manual_seed(5)
    x = torch.rand(per_node, k, generator=g)               # every node trains on the same samples
    if gn:
        Net = _gn_lenet(cin, h, w, c)
        x = x.reshape(per_node, cin, h, w)
    y = torch.randint(0, c, (per_node,), generator=g)
    runs = {}
    for flag in (False, True):
        torch.manual_seed(7)
        params = {"meta": {"log": "WARNING", "seed": 7}, "model": {"input-size": k},
                  "topology": {"name": "d-cliques", "remove-clique-edges": 0},
                  "logger": {"accuracy-logging-interval": 0, "accuracy-logging-interval-steps": 0,
                             "log-consensus-distance": False},
                  "algorithm": {"learning-rate": 0.01, "learning-momentum": a.momentum, "batch-size": b,
                                "initial-averaging": False, "clique-gradient": a.clique_gradient,
                                "unbiased-gradient": False, "deferred-writeback": True,
                                "mixing-mode": a.mode, "device-training": flag}}
        if gn and flag:
            params["algorithm"]["device-training-gn-lenet"] = True
        ts = [(x[j], int(y[j])) for j in range(per_node)]
        nodes = []
        for r in range(n):
            mdl = Net()
            nodes.append({"rank": r, "epoch": 0, "train-set": ts, "model": mdl,
                          "optimizer": d_sgd.optimizer(mdl, params)})
        state, _, _ = d_sgd.init(nodes, topo, params)
        runs[flag] = [state, params, []]
    for rnd in range(a.warmup + a.rounds):
        for flag in (False, True):
            state, params, times = runs[flag]
            t0 = time.perf_counter()
            state, losses, _, _ = d_sgd.next_step(state, params, None)
            d_sgd.synchronize()
            dt = time.perf_counter() - t0
            runs[flag][0] = state
            if rnd >= a.warmup:
                times.append(dt)
    out = {"step": "gn-rounds" if gn else "rounds", "shape": a.shape, "n": n, "k": k, "c": c, "b": b, "mode": a.mode,
           "clique_gradient": a.clique_gradient, "momentum": a.momentum,
           "warmup": a.warmup, "rounds": a.rounds, "threads": torch.get_num_threads(),
           "device": torch.cuda.get_device_name(0)}
    for flag, key in ((False, "flag_off"), (True, "flag_on")):
        t = runs[flag][2]
        out[key] = {"median_ms": statistics.median(t) * 1e3, "min_ms": min(t) * 1e3,
                    "max_ms": max(t) * 1e3}
    out["on_over_off"] = out["flag_on"]["median_ms"] / out["flag_off"]["median_ms"]
    print(json.dumps(out))


LARGE_SHAPES = ((1, 12800, 784, 10), (10, 6000, 784, 10), (100, 3277, 784, 10))
BOTH_SHAPES = ((1, 3276, 784, 10), (1000, 3276, 784, 10))


def _stats(t, nbytes=None):
    med = statistics.median(t)
    out = {"median_ms": med * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3}
    if nbytes is not None:
        out.update(bytes=nbytes, share_of_8TBps=nbytes / med / 8e12)
    return out


def _linear_calls(n, b, k, c, dev, pool=60000):
    """The two gradient entries on n rows with full batches of b samples drawn from a pool:
    ({name: call}, bytes the sliced call must move, loss)."""
    import torch
    from niidmix import _lib, train
    lib = _lib.lib
    p = c * k + c
    ld = train.padded_ld(p)
    gen = torch.Generator(device=dev).manual_seed(1)
    theta = (torch.rand(n, ld, device=dev, generator=gen) - 0.5) * (2 / k ** 0.5)
    grad = torch.zeros(n, ld, device=dev)
    data = torch.rand(pool, k, device=dev, generator=gen)
    labels = torch.randint(0, c, (pool,), device=dev, generator=gen).to(torch.int32)
    idx = torch.randint(0, pool, (n, b), device=dev, generator=gen).to(torch.int32).contiguous()
    blen = torch.full((n,), b, dtype=torch.int32, device=dev)
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    loss = torch.empty(n, device=dev)
    strm = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    calls = {}
    for name, fn, elems in (
            ("sliced", lib.niidmix_linear_nll_grad_rows_sliced_f32,
             int(lib.niidmix_linear_nll_grad_rows_sliced_scratch_elems(n, b, k, c))),
            ("existing", lib.niidmix_linear_nll_grad_rows_f32,
             int(lib.niidmix_linear_nll_grad_rows_scratch_elems(n, b, c)) if b * c <= 32768 else None)):
        if elems is None:
            continue
        scratch = torch.empty(elems, device=dev)
        calls[name] = lambda fn=fn, scratch=scratch, elems=elems: fn(
            theta.data_ptr(), ld, data.data_ptr(), labels.data_ptr(), idx.data_ptr(), blen.data_ptr(), b,
            rows.data_ptr(), n, grad.data_ptr(), ld, loss.data_ptr(), k, c, scratch.data_ptr(), elems, strm)
    n_sl = -(-b // int(lib.niidmix_linear_nll_grad_rows_sliced_slice(c)))
    n_kc = min(8, -(-1024 // n), -(-k // 256))
    # the gather of x twice, the partial logits written and read and dz written and read, the partial
    # gradients written and read, theta read and grad written
    nbytes = 4 * (2 * n * b * k + 2 * (n_kc + 1) * n * b * c + 2 * n * n_sl * p + 2 * n * p)
    return calls, nbytes, loss


def _alternate(calls, a):
    """Device-event times of single calls, alternating within every repetition."""
    import torch
    from niidmix import _lib
    times = {name: [] for name in calls}
    for rep in range(a.warmup + a.reps):
        for name, fn in calls.items():
            s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            _lib.check(fn(), name)
            e0.record()
            e0.synchronize()
            if rep >= a.warmup:
                times[name].append(s0.elapsed_time(e0) * 1e-3)
    return times


def _passes(call, a):
    """Device time of each kernel of one call, by torch's profiler: {kernel: stats} or a reason."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    try:
        per = {}
        for _ in range(a.reps):
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                call()
                torch.cuda.synchronize()
            for ev in prof.events():
                m = re.search(r"k_lin_\w+", ev.name)
                if m and ev.device_time_total > 0:
                    per.setdefault(m.group(0), []).append(ev.device_time_total * 1e-6)
        return {k: _stats(v) for k, v in per.items()} or "the profiler recorded no k_lin_ kernel"
    except Exception as e:                     # a measurement aid: the totals above stand without it
        return f"{type(e).__name__}: {e}"


def large_batch(a):
    """--device-training-large-batch: the sliced call at few rows and long batches (the four passes
    apart at the first shape), the sliced against the existing entry at the largest batch both
    take, and the centralised round (one node, 60 000 x 784 synthetic samples, batch 12 800) under
    the flag with --device-sampling-cached against the same round with every device flag off."""
    import torch
    import torch.nn.functional as F
    from niidmix import _lib, d_sgd
    dev = torch.device("cuda:0")
    out = {"step": "large-batch", "warmup": a.warmup, "reps": a.reps, "threads": torch.get_num_threads(),
           "device": torch.cuda.get_device_name(dev), "lib_sha16": _lib.lib_sha16(), "sliced": [], "both": []}
    for i, (n, b, k, c) in enumerate(LARGE_SHAPES):
        calls, nbytes, loss = _linear_calls(n, b, k, c, dev)
        t = _alternate({"sliced": calls["sliced"]}, a)
        assert bool(torch.isfinite(loss).all())
        rec = {"shape": [n, b, k, c], **_stats(t["sliced"], nbytes)}
        if i == 0:
            rec["passes"] = _passes(calls["sliced"], a)
        out["sliced"].append(rec)
    for n, b, k, c in BOTH_SHAPES:
        calls, nbytes, loss = _linear_calls(n, b, k, c, dev)
        t = _alternate(calls, a)
        assert bool(torch.isfinite(loss).all())
        rec = {"shape": [n, b, k, c], **{name: _stats(v) for name, v in t.items()}}
        rec["sliced_over_existing"] = rec["sliced"]["median_ms"] / rec["existing"]["median_ms"]
        out["both"].append(rec)

    k, c, b, size = 784, 10, 12800, 60000

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = torch.nn.Linear(k, c)

        def forward(self, x, params):
            return F.log_softmax(self.fc(x.view(-1, k)), dim=1)

    g = torch.Generator().manual_seed(5)
    x = torch.rand(size, k, generator=g)
    y = torch.randint(0, c, (size,), generator=g)
    ts = [(x[j], int(y[j])) for j in range(size)]
    topo = {"edges": {0: []}, "weights": torch.tensor([[1.0]])}
    flags = {"device-training": True, "device-training-large-batch": True, "device-sampling": True,
             "device-sampling-cached": True}
    runs = {}
    for name, extra in (("flags_off", {}), ("flagged", flags)):
        torch.manual_seed(7)
        params = {"meta": {"log": "WARNING", "seed": 7}, "model": {"input-size": k},
                  "topology": {"name": "fully-connected", "remove-clique-edges": 0},
                  "logger": {"accuracy-logging-interval": 0, "accuracy-logging-interval-steps": 0,
                             "log-consensus-distance": False},
                  "algorithm": {"learning-rate": 0.01, "learning-momentum": 0.0, "batch-size": b,
                                "initial-averaging": False, "clique-gradient": False,
                                "unbiased-gradient": False, "deferred-writeback": True,
                                "mixing-mode": a.mode, **extra}}
        mdl = Net()
        nodes = [{"rank": 0, "epoch": 0, "train-set": ts, "model": mdl,
                  "optimizer": d_sgd.optimizer(mdl, params)}]
        state, _, _ = d_sgd.init(nodes, topo, params)
        runs[name] = [state, params, []]
    for rnd in range(a.warmup + a.reps):
        for name in runs:
            state, params, times = runs[name]
            t0 = time.perf_counter()
            state, _, _, _ = d_sgd.next_step(state, params, None)
            d_sgd.synchronize()
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            runs[name][0] = state
            if rnd >= a.warmup:
                times.append(dt)
    out["centralised_round"] = {"samples": size, "k": k, "c": c, "batch": b,
                                **{name: _stats(r[2]) for name, r in runs.items()}}
    out["centralised_round"]["flagged_over_off"] = \
        out["centralised_round"]["flagged"]["median_ms"] / out["centralised_round"]["flags_off"]["median_ms"]
    print(json.dumps(out))


def run_all(a):
    for step in ("kernel", "rounds"):
        for shape in SHAPES:
            cmd = [sys.executable, os.path.abspath(__file__), step, "--shape", shape]
            print("+", " ".join(cmd[1:]), flush=True)
            rc = subprocess.run(cmd, timeout=STEP_LIMIT_S[step]).returncode
            if rc != 0:
                sys.exit(f"device_training_probe: {step} {shape} ended with status {rc}; stopping")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=["kernel", "rounds", "gn-kernel", "gn-rounds", "fused-step", "large-batch",
                                     "all"])
    ap.add_argument("--shape", choices=list(SHAPES) + list(GN_SHAPES), default=None)
    ap.add_argument("--loop-nodes-device", type=int, default=8,
                    help="gn-kernel: nodes the device autograd loop runs per repetition (scaled to N)")
    ap.add_argument("--loop-nodes-cpu", type=int, default=3,
                    help="gn-kernel: nodes the CPU loop runs per repetition (scaled to N)")
    ap.add_argument("--nodes", type=int, default=0, help="override the shape's node count")
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--mode", choices=["exact", "fast"], default="exact")
    ap.add_argument("--clique-gradient", action="store_true",
                    help="rounds / gn-rounds: both paths average the cliques' gradients")
    ap.add_argument("--momentum", type=float, default=0.0, help="rounds / gn-rounds: --learning-momentum")
    a = ap.parse_args()
    if a.step == "all":
        return run_all(a)
    import torch
    if not torch.cuda.is_available():
        sys.exit("device_training_probe: no GPU (a rate is only ever measured on one)")
    gn = a.step.startswith("gn-")
    if a.warmup is None:
        a.warmup = 2 if a.step.endswith("rounds") else 5
    if a.step == "large-batch":
        return large_batch(a)
    if a.step == "fused-step":
        a.shape = a.shape or "e2e"
        if a.shape not in ("e2e", "gn-cifar"):
            sys.exit(f"device_training_probe: fused-step takes the shapes e2e and gn-cifar, not {a.shape}")
        return fused_step(a)
    if a.shape is None:
        a.shape = "gn-cifar" if gn else "ref"
    if (a.shape in GN_SHAPES) != gn:
        sys.exit(f"device_training_probe: {a.step} does not take the shape {a.shape}")
    {"kernel": kernel, "rounds": rounds, "gn-kernel": gn_kernel, "gn-rounds": rounds}[a.step](a)


if __name__ == "__main__":
    main()
