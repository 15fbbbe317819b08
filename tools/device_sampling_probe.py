#!/usr/bin/env python
"""Device-sampling probe (measurement tool): what niidmix_draw_batches_i32 and a round under
--device-sampling cost on one GPU.

  kernel   device-event times of single launches of the draw (every job at cursor 0 of epoch 0)
           and of the linear model's gradient call on the batches it drew (K 784, C 10),
           alternating within every repetition, at
               small   N 1000, segments of 60 samples,  B 125
               large   N 100,  segments of 600 samples, B 128
  rounds   d_sgd.next_step + synchronise with --device-sampling on and off (off: the same
           device-training round on DataLoader draws, the behaviour without the flag),
           interleaved round by round in one process after a warm-up; median, minimum and
           maximum of each and their ratio.  The plugin keeps one device trainer alive, so the
           probe holds both runs' trainers and puts each back before its round.
               linear   1000 nodes, Linear(784, 10), batch 125, d-cliques of 100 (--device-training)
               sample   the same nodes on the 'sample' topology, sample-size 100
                        (--device-training-sample)
               gn       1000 GN-LeNet nodes, 3 x 32 x 32, batch 20 (--device-training-gn-lenet)
           Then, on the flag-on trainer, what stays on the host in such a round, each alone
           between two synchronises (median): the slab's write-back, the loss copy, and
           SamplerState.advance.
           --per-node sets every node's train-set length (default 2 x batch; 60 with batch 125
           makes every round an epoch, as MNIST over 1000 nodes does).
           --cached compares the two sampling modes instead: flag off is plain --device-sampling,
           flag on adds --device-sampling-cached.
  cached   device-event times of single launches, alternating within every repetition, of
           niidmix_epoch_perm_i32 (every job's epoch 0), niidmix_take_batches_i32 at cursor 0,
           the stateless draw where the segments allow it (up to 8192 samples) and the linear
           gradient call on the batches taken, at the two shapes above and
               e60000  1 job of 60 000 samples, B 128
               e10000  5 jobs of 10 000 samples, B 128
           and epoch_perm's share of the gradient call once divided by the rounds of an epoch.
  torch    the same for niidmix_torch_randperm_i32 (--device-sampling-torch-stream): single
           launches of it, of niidmix_epoch_perm_i32 on the same jobs and of
           niidmix_take_batches_i32, alternating, checked against torch.randperm on the CPU, at
               r250    1000 jobs of 250 samples, B 125
               e60000  1 job of 60 000 samples, B 128
           rounds --torch-stream compares whole rounds: flag off is --device-sampling
           --device-sampling-cached, flag on adds --device-sampling-torch-stream.

    python tools/device_sampling_probe.py kernel --shape small [--warmup 5] [--reps 20]
    python tools/device_sampling_probe.py rounds --run linear [--per-node 60] [--warmup 2] [--rounds 10]
    python tools/device_sampling_probe.py rounds --run linear --cached
    python tools/device_sampling_probe.py cached --shape e60000 [--warmup 5] [--reps 20]
    python tools/device_sampling_probe.py torch --shape r250 [--warmup 5] [--reps 20]
    python tools/device_sampling_probe.py rounds --run linear --torch-stream --per-node 250

Every step prints one JSON line.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "non-iid-topology-simulator_amd"), os.path.join(REPO, "tools")]

KERNEL_SHAPES = {"small": (1000, 60, 125), "large": (100, 600, 128)}
CACHED_SHAPES = {**KERNEL_SHAPES, "e60000": (1, 60000, 128), "e10000": (5, 10000, 128)}
TORCH_SHAPES = {"r250": (1000, 250, 125), "e60000": CACHED_SHAPES["e60000"]}
K, C = 784, 10


def _stats(t):
    return {"median_ms": statistics.median(t) * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3}


def kernel(a):
    import numpy as np
    import torch
    from niidmix import _lib, sampling, train
    n, length, b = KERNEL_SHAPES[a.shape]
    dev = torch.device("cuda:0")
    p = C * K + C
    ld = train.padded_ld(p)
    gen = torch.Generator(device=dev).manual_seed(1)
    theta = (torch.rand(n, ld, device=dev, generator=gen) - 0.5) * (2 / K ** 0.5)
    grad = torch.zeros(n, ld, device=dev)
    data = torch.rand(n * length, K, device=dev, generator=gen)
    labels = torch.randint(0, C, (n * length,), device=dev, generator=gen).to(torch.int32)
    i32 = dict(dtype=torch.int32, device=dev)
    rank = torch.arange(n, **i32)
    start, seg = rank * length, torch.full((n,), length, **i32)
    zero = torch.zeros(n, **i32)
    idx, blen = torch.zeros(n, b, **i32), torch.zeros(n, **i32)
    loss = torch.empty(n, device=dev)
    lib = _lib.lib
    elems = int(lib.niidmix_linear_nll_grad_rows_scratch_elems(n, b, C))
    scratch = torch.empty(elems, device=dev)
    strm = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def draw_call():
        return lib.niidmix_draw_batches_i32(a.seed, rank.data_ptr(), start.data_ptr(), seg.data_ptr(),
                                            zero.data_ptr(), zero.data_ptr(), n, b, idx.data_ptr(),
                                            blen.data_ptr(), strm)

    def grad_call():
        return lib.niidmix_linear_nll_grad_rows_f32(
            theta.data_ptr(), ld, data.data_ptr(), labels.data_ptr(), idx.data_ptr(), blen.data_ptr(),
            b, rank.data_ptr(), n, grad.data_ptr(), ld, loss.data_ptr(), K, C, scratch.data_ptr(),
            elems, strm)

    calls = [("draw", draw_call), ("grad", grad_call)]
    times = {name: [] for name, _ in calls}
    for rep in range(a.warmup + a.reps):
        for name, fn in calls:
            s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            _lib.check(fn(), name)
            e0.record()
            e0.synchronize()
            if rep >= a.warmup:
                times[name].append(s0.elapsed_time(e0) * 1e-3)
    nb = min(b, length)
    got = idx.cpu().numpy()
    for r in (0, n - 1):                                   # what was timed is the stream
        want = r * length + sampling.epoch_permutation(a.seed, r, 0, length)[:nb]
        assert np.array_equal(got[r, :nb], want), r
    assert bool((blen == nb).all()) and bool(torch.isfinite(loss).all())
    out = {"step": "kernel", "shape": a.shape, "n": n, "len": length, "b": b, "k": K, "c": C,
           "warmup": a.warmup, "reps": a.reps, "device": torch.cuda.get_device_name(dev),
           "lib_sha16": _lib.lib_sha16()}
    for name, _ in calls:
        out[name] = _stats(times[name])
    out["draw_over_grad"] = out["draw"]["median_ms"] / out["grad"]["median_ms"]
    print(json.dumps(out))


def cached(a):
    import numpy as np
    import torch
    from niidmix import _lib, sampling, train
    n, length, b = CACHED_SHAPES[a.shape]
    dev = torch.device("cuda:0")
    ld = train.padded_ld(C * K + C)
    gen = torch.Generator(device=dev).manual_seed(1)
    theta = (torch.rand(n, ld, device=dev, generator=gen) - 0.5) * (2 / K ** 0.5)
    grad = torch.zeros(n, ld, device=dev)
    data = torch.rand(n * length, K, device=dev, generator=gen)
    labels = torch.randint(0, C, (n * length,), device=dev, generator=gen).to(torch.int32)
    i32 = dict(dtype=torch.int32, device=dev)
    rank = torch.arange(n, **i32)
    start, seg = rank * length, torch.full((n,), length, **i32)
    off = start.to(torch.int64)
    zero = torch.zeros(n, **i32)
    idx, blen = torch.zeros(n, b, **i32), torch.zeros(n, **i32)
    idx2, blen2 = torch.zeros(n, b, **i32), torch.zeros(n, **i32)
    perm = torch.zeros(n * length, **i32)
    loss = torch.empty(n, device=dev)
    lib = _lib.lib
    elems = int(lib.niidmix_linear_nll_grad_rows_scratch_elems(n, b, C))
    scratch = torch.empty(elems, device=dev)
    sort_bytes = int(lib.niidmix_epoch_perm_scratch_bytes(n, length))
    sort_scratch = torch.empty(max(sort_bytes // 8, 2), dtype=torch.int64, device=dev)
    strm = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def perm_call():
        return lib.niidmix_epoch_perm_i32(a.seed, rank.data_ptr(), seg.data_ptr(), zero.data_ptr(),
                                          off.data_ptr(), n, length, perm.data_ptr(), perm.numel(),
                                          sort_scratch.data_ptr(), sort_bytes, strm)

    def take_call():
        return lib.niidmix_take_batches_i32(perm.data_ptr(), perm.numel(), off.data_ptr(), start.data_ptr(),
                                            seg.data_ptr(), zero.data_ptr(), n, b, idx.data_ptr(),
                                            blen.data_ptr(), strm)

    def draw_call():
        return lib.niidmix_draw_batches_i32(a.seed, rank.data_ptr(), start.data_ptr(), seg.data_ptr(),
                                            zero.data_ptr(), zero.data_ptr(), n, b, idx2.data_ptr(),
                                            blen2.data_ptr(), strm)

    def grad_call():
        return lib.niidmix_linear_nll_grad_rows_f32(
            theta.data_ptr(), ld, data.data_ptr(), labels.data_ptr(), idx.data_ptr(), blen.data_ptr(),
            b, rank.data_ptr(), n, grad.data_ptr(), ld, loss.data_ptr(), K, C, scratch.data_ptr(),
            elems, strm)

    stateless = length <= int(lib.niidmix_draw_batches_max_len())
    calls = [("epoch_perm", perm_call), ("take", take_call)] + ([("draw", draw_call)] if stateless else []) + \
        [("grad", grad_call)]
    times = {name: [] for name, _ in calls}
    for rep in range(a.warmup + a.reps):
        for name, fn in calls:
            s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            _lib.check(fn(), name)
            e0.record()
            e0.synchronize()
            if rep >= a.warmup:
                times[name].append(s0.elapsed_time(e0) * 1e-3)
    nb = min(b, length)
    got, whole = idx.cpu().numpy(), perm.cpu().numpy()
    for r in (0, n - 1):                                   # what was timed is the stream
        want = sampling.epoch_permutation(a.seed, r, 0, length)
        assert np.array_equal(whole[r * length:(r + 1) * length], want), r
        assert np.array_equal(got[r, :nb], r * length + want[:nb]), r
    assert bool((blen == nb).all()) and bool(torch.isfinite(loss).all())
    assert not stateless or (torch.equal(idx2[:, :nb], idx[:, :nb]) and torch.equal(blen2, blen))
    rounds_per_epoch = -(-length // b)
    out = {"step": "cached", "shape": a.shape, "n": n, "len": length, "b": b, "k": K, "c": C,
           "warmup": a.warmup, "reps": a.reps, "device": torch.cuda.get_device_name(dev),
           "lib_sha16": _lib.lib_sha16(), "rounds_per_epoch": rounds_per_epoch}
    for name, _ in calls:
        out[name] = _stats(times[name])
    out["epoch_perm_per_round_over_grad"] = out["epoch_perm"]["median_ms"] / rounds_per_epoch / \
        out["grad"]["median_ms"]
    if stateless:
        out["take_over_draw"] = out["take"]["median_ms"] / out["draw"]["median_ms"]
    print(json.dumps(out))


def torch_stream(a):
    import numpy as np
    import torch
    from niidmix import _lib
    n, length, b = TORCH_SHAPES[a.shape]
    dev = torch.device("cuda:0")
    i32 = dict(dtype=torch.int32, device=dev)
    rank = torch.arange(n, **i32)
    seeds = rank + a.seed                                  # job j: manual_seed(seed + j)
    start, seg = rank * length, torch.full((n,), length, **i32)
    off = start.to(torch.int64)
    zero = torch.zeros(n, **i32)
    idx, blen = torch.zeros(n, b, **i32), torch.zeros(n, **i32)
    perm, perm2 = torch.zeros(n * length, **i32), torch.zeros(n * length, **i32)
    lib = _lib.lib
    sort_bytes = int(lib.niidmix_epoch_perm_scratch_bytes(n, length))
    sort_scratch = torch.empty(max(sort_bytes // 8, 2), dtype=torch.int64, device=dev)
    strm = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def shuffle_call():
        return lib.niidmix_torch_randperm_i32(seeds.data_ptr(), seg.data_ptr(), off.data_ptr(), n, length,
                                              perm.data_ptr(), perm.numel(), strm)

    def sort_call():
        return lib.niidmix_epoch_perm_i32(a.seed, rank.data_ptr(), seg.data_ptr(), zero.data_ptr(),
                                          off.data_ptr(), n, length, perm2.data_ptr(), perm2.numel(),
                                          sort_scratch.data_ptr(), sort_bytes, strm)

    def take_call():
        return lib.niidmix_take_batches_i32(perm.data_ptr(), perm.numel(), off.data_ptr(), start.data_ptr(),
                                            seg.data_ptr(), zero.data_ptr(), n, b, idx.data_ptr(),
                                            blen.data_ptr(), strm)

    calls = [("torch_randperm", shuffle_call), ("epoch_perm", sort_call), ("take", take_call)]
    times = {name: [] for name, _ in calls}
    for rep in range(a.warmup + a.reps):
        for name, fn in calls:
            s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            _lib.check(fn(), name)
            e0.record()
            e0.synchronize()
            if rep >= a.warmup:
                times[name].append(s0.elapsed_time(e0) * 1e-3)
    nb = min(b, length)
    got, whole = idx.cpu().numpy(), perm.cpu().numpy()
    for r in (0, n - 1):                                   # what was timed is torch's permutation
        want = torch.randperm(length, generator=torch.Generator().manual_seed(a.seed + r)).numpy()
        assert np.array_equal(whole[r * length:(r + 1) * length], want), r
        assert np.array_equal(got[r, :nb], r * length + want[:nb]), r
    rounds_per_epoch = -(-length // b)
    out = {"step": "torch", "shape": a.shape, "n": n, "len": length, "b": b, "warmup": a.warmup,
           "reps": a.reps, "device": torch.cuda.get_device_name(dev), "lib_sha16": _lib.lib_sha16(),
           "rounds_per_epoch": rounds_per_epoch}
    for name, _ in calls:
        out[name] = _stats(times[name])
    out["torch_randperm_over_epoch_perm"] = out["torch_randperm"]["median_ms"] / out["epoch_perm"]["median_ms"]
    out["torch_randperm_us_per_round"] = out["torch_randperm"]["median_ms"] * 1e3 / rounds_per_epoch
    print(json.dumps(out))


def rounds(a):
    import torch
    import torch.nn.functional as F
    from niidmix import d_sgd
    from niidmix.generate import dcliques
    from niidmix.topology import mh_csr
    n = a.nodes
    gn = a.run == "gn"
    b = a.batch or (20 if gn else 125)
    per_node = a.per_node or 2 * b
    k = 3 * 32 * 32 if gn else K

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = torch.nn.Linear(k, C)

        def forward(self, x, params):
            return F.log_softmax(self.fc(x.view(-1, k)), dim=1)

    g = torch.Generator().manual_seed(5)
    x = torch.rand(per_node, k, generator=g)               # every node trains on the same samples
    if gn:
        from device_training_probe import _gn_lenet
        Net = _gn_lenet(3, 32, 32, C)
        x = x.reshape(per_node, 3, 32, 32)
    y = torch.randint(0, C, (per_node,), generator=g)
    ts = [(x[j], int(y[j])) for j in range(per_node)]
    if a.run == "sample":
        topo = {"edges": {}, "weights": []}
        tparams = {"name": "sample", "sample-method": "random", "sample-size": a.sample}
    else:
        edges, cliques = dcliques(n, min(100, n), "fully-connected", 1337)
        topo = {"edges": edges, "csr": mh_csr(n, edges), "weights": torch.tensor([]), "cliques": cliques}
        tparams = {"name": "d-cliques", "remove-clique-edges": 0}
    flags = {"linear": (), "sample": ("device-training-sample",), "gn": ("device-training-gn-lenet",)}[a.run]
    runs = {}
    for on in (False, True):
        torch.manual_seed(7)
        params = {"meta": {"log": "WARNING", "seed": 7}, "model": {"input-size": k},
                  "topology": dict(tparams),
                  "logger": {"accuracy-logging-interval": 0, "accuracy-logging-interval-steps": 0,
                             "log-consensus-distance": False},
                  "algorithm": {"learning-rate": 0.01, "learning-momentum": a.momentum, "batch-size": b,
                                "initial-averaging": False, "clique-gradient": False,
                                "unbiased-gradient": False, "deferred-writeback": True,
                                "mixing-mode": "exact", "device-training": True,
                                **{f: True for f in flags},
                                **({"device-sampling": True} if on or a.cached or a.torch_stream else {}),
                                **({"device-sampling-cached": True} if (on and a.cached) or a.torch_stream
                                   else {}),
                                **({"device-sampling-torch-stream": True} if on and a.torch_stream else {})}}
        nodes = []
        for r in range(n):
            mdl = Net()
            nodes.append({"rank": r, "epoch": 0, "train-set": ts, "model": mdl,
                          "optimizer": d_sgd.optimizer(mdl, params)})
        state, _, _ = d_sgd.init(nodes, topo, params)
        runs[on] = {"state": state, "params": params, "times": [], "trainer": None}
    for rnd in range(a.warmup + a.rounds):
        for on in (False, True):
            run = runs[on]
            d_sgd._trainers.clear()                        # the plugin keeps one trainer: this run's
            if run["trainer"] is not None:
                d_sgd._trainers[id(run["state"]["nodes"])] = run["trainer"]
            t0 = time.perf_counter()
            run["state"], losses, _, _ = d_sgd.next_step(run["state"], run["params"], None)
            d_sgd.synchronize()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            run["trainer"] = d_sgd._trainers[id(run["state"]["nodes"])]
            tr = run["trainer"]
            assert tr.sampling == (on or a.cached or a.torch_stream) and tr.torch_stream == (on and a.torch_stream)
            assert tr.cached == ((on and a.cached) or a.torch_stream)
            if rnd >= a.warmup:
                run["times"].append(dt)
    out = {"step": "rounds", "run": a.run, "cached": a.cached, "torch_stream": a.torch_stream, "n": n, "k": k, "c": C, "b": b, "per_node": per_node,
           "sample": a.sample if a.run == "sample" else None, "momentum": a.momentum,
           "warmup": a.warmup, "rounds": a.rounds, "threads": torch.get_num_threads(),
           "device": torch.cuda.get_device_name(0)}
    out["flag_off"], out["flag_on"] = _stats(runs[False]["times"]), _stats(runs[True]["times"])
    out["on_over_off"] = out["flag_on"]["median_ms"] / out["flag_off"]["median_ms"]
    out["on_median_within_off_spread"] = \
        out["flag_off"]["min_ms"] <= out["flag_on"]["median_ms"] <= out["flag_off"]["max_ms"]
    # what is left on the host in a flag-on round, each alone between two synchronises: the
    # synchronous write-back of the slab, the loss copy, and the sampler's host part
    tr, parts = runs[True]["trainer"], {"write_back": [], "loss_d2h": [], "advance": []}
    rows = list(range(min(a.sample, n))) if a.run == "sample" else tr.source.all_rows
    for _ in range(a.rounds):
        for name, fn in (("write_back", tr.write_back), ("loss_d2h", lambda: tr.loss.cpu().tolist()),
                         ("advance", lambda: tr.source.sampler.advance(rows))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            parts[name].append(time.perf_counter() - t0)
    out["flag_on_parts_ms"] = {name: statistics.median(t) * 1e3 for name, t in parts.items()}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=["kernel", "rounds", "cached", "torch"])
    ap.add_argument("--shape", choices=list({**CACHED_SHAPES, **TORCH_SHAPES}), default="small")
    ap.add_argument("--torch-stream", action="store_true",
                    help="rounds: flag off is --device-sampling --device-sampling-cached, flag on adds "
                         "--device-sampling-torch-stream")
    ap.add_argument("--cached", action="store_true",
                    help="rounds: flag off is plain --device-sampling, flag on adds --device-sampling-cached")
    ap.add_argument("--run", choices=["linear", "sample", "gn"], default="linear")
    ap.add_argument("--nodes", type=int, default=1000)
    ap.add_argument("--sample", type=int, default=100, help="rounds --run sample: the sample size")
    ap.add_argument("--batch", type=int, default=0, help="rounds: batch size (125; gn: 20)")
    ap.add_argument("--per-node", type=int, default=0, help="rounds: samples per node (2 x batch)")
    ap.add_argument("--momentum", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("device_sampling_probe: no GPU (a time is only ever measured on one)")
    if a.warmup is None:
        a.warmup = 2 if a.step == "rounds" else 5
    if a.step == "kernel" and a.shape not in KERNEL_SHAPES:
        sys.exit(f"device_sampling_probe: kernel --shape is one of {list(KERNEL_SHAPES)}")
    if a.step == "cached" and a.shape not in CACHED_SHAPES:
        sys.exit(f"device_sampling_probe: cached --shape is one of {list(CACHED_SHAPES)}")
    if a.step == "torch" and a.shape not in TORCH_SHAPES:
        sys.exit(f"device_sampling_probe: torch --shape is one of {list(TORCH_SHAPES)}")
    {"kernel": kernel, "rounds": rounds, "cached": cached, "torch": torch_stream}[a.step](a)


if __name__ == "__main__":
    main()
