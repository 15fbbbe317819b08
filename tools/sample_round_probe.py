#!/usr/bin/env python
"""Timings behind DESIGN §5 "The sample round" (--device-training-sample), on one GPU.

  kernel   niidmix_sample_step_mean_update_f32 (one launch) against the three calls it restates
           (niidmix_sgd_step_rows_f32 or niidmix_sgd_momentum_step_rows_f32, niidmix_mix_csr_f32 with
           EXACT | AVERAGE_ONLY, niidmix_update_rows_f32) and niidmix_stream_copy_f32 over the same
           slab, alternating in one process: device events, --warmup repetitions, then median,
           minimum and maximum of --reps.  Momentum 0 and steady-state momentum (no first step).
           Reported with the algorithmic bytes (include/niidmix.h) as a rate and as a fraction of
           the stream copy's rate in the same run.
  rounds   d_sgd.next_step on a sample run of --nodes linear models (784 x 10, batch 125,
           sample-size 100, method random), flag on and flag off interleaved, host clock around a
           round that ends in d_sgd.synchronize().

    python tools/sample_round_probe.py kernel --nodes 1000 --sample 100 --cols 1048576
    python tools/sample_round_probe.py rounds --nodes 1000 --sample 100

One JSON line per call.  A job that runs several of them gives each its own `timeout -k 10` and
chains them with `&&`."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "non-iid-topology-simulator_amd"))


def kernel(a):
    import numpy as np
    import torch
    from niidmix import _lib, ops, train
    n, k, p = a.nodes, a.sample, a.cols
    ld = train.padded_ld(p)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    x, g, buf = (torch.randn(n, ld, device=dev, generator=gen) for _ in range(3))
    y = torch.empty(n, ld, device=dev)
    active = torch.randperm(n, device=dev, generator=gen)[:k].to(torch.int32).contiguous()
    first = torch.zeros(k, dtype=torch.int32, device=dev)
    row_ptr = torch.tensor([0, k], dtype=torch.int64, device=dev)
    w = float(np.float32(1.0 / k))
    val = torch.full((k,), w, dtype=torch.float32, device=dev)
    avg = torch.empty(ld, device=dev)
    lib, lr = _lib.lib, -1e-3
    strm = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def fused(m):
        return lib.niidmix_sample_step_mean_update_f32(
            x.data_ptr(), ld, y.data_ptr(), ld, g.data_ptr(), ld, buf.data_ptr() if m else None,
            ld if m else 0, active.data_ptr(), first.data_ptr() if m else None, w, lr, m, p, n, k, strm)

    def parts(m):
        if m:
            rc = lib.niidmix_sgd_momentum_step_rows_f32(x.data_ptr(), ld, g.data_ptr(), ld, buf.data_ptr(),
                                                        ld, p, active.data_ptr(), k, lr, m, 0, strm)
        else:
            rc = lib.niidmix_sgd_step_rows_f32(x.data_ptr(), ld, g.data_ptr(), ld, p, active.data_ptr(), k,
                                               lr, strm)
        rc = rc or lib.niidmix_mix_csr_f32(x.data_ptr(), ld, avg.data_ptr(), ld, 1, p, row_ptr.data_ptr(),
                                           active.data_ptr(), val.data_ptr(),
                                           ops.EXACT | ops.AVERAGE_ONLY, strm)
        return rc or lib.niidmix_update_rows_f32(x.data_ptr(), ld, y.data_ptr(), ld, n, p, avg.data_ptr(), strm)

    def copy(m):
        return lib.niidmix_stream_copy_f32(x.data_ptr(), y.data_ptr(), n * ld, strm)

    # bytes per column: include/niidmix.h, niidmix_sample_step_mean_update_f32
    cands = [("copy", copy, 0.0, 2 * n), ("fused_m0", fused, 0.0, 2 * n + 2 * k),
             ("parts_m0", parts, 0.0, 2 * n + 4 * k), ("fused_m09", fused, 0.9, 2 * n + 4 * k),
             ("parts_m09", parts, 0.9, 2 * n + 6 * k)]
    times = {name: [] for name, _, _, _ in cands}
    for r in range(a.warmup + a.reps):
        for name, fn, m, _ in cands:
            s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            _lib.check(fn(m), name)
            e0.record()
            e0.synchronize()
            if r >= a.warmup:
                times[name].append(s0.elapsed_time(e0) * 1e-3)
    out = {"step": "kernel", "n": n, "k": k, "p": p, "ld": ld, "warmup": a.warmup, "reps": a.reps,
           "device": torch.cuda.get_device_name(dev), "lib_sha16": _lib.lib_sha16()}
    for name, _, _, words in cands:
        t = times[name]
        med = statistics.median(t)
        out[name] = {"bytes": 4 * words * p, "median_us": med * 1e6, "min_us": min(t) * 1e6,
                     "max_us": max(t) * 1e6, "gbps_median": 4 * words * p / med / 1e9}
    for name, _, _, _ in cands[1:]:
        out[name]["fraction_of_copy_rate"] = out[name]["gbps_median"] / out["copy"]["gbps_median"]
    for tag in ("m0", "m09"):
        f, s = out["fused_" + tag], out["parts_" + tag]
        out["fused_over_parts_" + tag] = f["median_us"] / s["median_us"]
        out["fused_slower_beyond_spread_" + tag] = f["median_us"] - s["median_us"] > s["max_us"] - s["min_us"]
    print(json.dumps(out))


def rounds(a):
    import torch
    import torch.nn.functional as F
    from niidmix import d_sgd
    n, kk, c, b = a.nodes, 784, 10, 125
    per_node = 2 * b

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = torch.nn.Linear(kk, c)

        def forward(self, x, params):
            return F.log_softmax(self.fc(x.view(-1, kk)), dim=1)

    g = torch.Generator().manual_seed(5)
    x = torch.rand(per_node, kk, generator=g)               # every node trains on the same samples
    y = torch.randint(0, c, (per_node,), generator=g)
    ts = [(x[j], int(y[j])) for j in range(per_node)]
    runs = {}
    for flag in (False, True):
        torch.manual_seed(7)
        params = {"meta": {"log": "WARNING", "seed": 7}, "model": {"input-size": kk},
                  "topology": {"name": "sample", "sample-method": "random", "sample-size": a.sample},
                  "logger": {"accuracy-logging-interval": 0, "accuracy-logging-interval-steps": 0,
                             "log-consensus-distance": False},
                  "algorithm": {"learning-rate": 0.01, "learning-momentum": a.momentum, "batch-size": b,
                                "initial-averaging": False, "clique-gradient": False,
                                "unbiased-gradient": False, "deferred-writeback": True,
                                "mixing-mode": "exact"}}
        if flag:
            params["algorithm"].update({"device-training": True, "device-training-sample": True})
        nodes = []
        for r in range(n):
            mdl = Net()
            nodes.append({"rank": r, "epoch": 0, "train-set": ts, "model": mdl,
                          "optimizer": d_sgd.optimizer(mdl, params)})
        state, _, _ = d_sgd.init(nodes, {"edges": {}, "weights": []}, params)
        runs[flag] = [state, params, []]
    for rnd in range(a.warmup + a.rounds):
        for flag in (False, True):
            state, params, times = runs[flag]
            t0 = time.perf_counter()
            state, _, _, _ = d_sgd.next_step(state, params, None)
            d_sgd.synchronize()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            runs[flag][0] = state
            if rnd >= a.warmup:
                times.append(dt)
    tr = d_sgd._trainers[id(runs[True][0]["nodes"])]
    out = {"step": "rounds", "n": n, "k": kk, "c": c, "b": b, "sample": a.sample, "momentum": a.momentum,
           "warmup": a.warmup, "rounds": a.rounds, "threads": torch.get_num_threads(),
           "one_launch": tr.sample_fused, "device": torch.cuda.get_device_name(0)}
    for flag, key in ((False, "flag_off"), (True, "flag_on")):
        t = runs[flag][2]
        out[key] = {"median_ms": statistics.median(t) * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3}
    out["off_over_on"] = out["flag_off"]["median_ms"] / out["flag_on"]["median_ms"]
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=["kernel", "rounds"])
    ap.add_argument("--nodes", type=int, default=1000)
    ap.add_argument("--sample", type=int, default=100)
    ap.add_argument("--cols", type=int, default=1 << 20)
    ap.add_argument("--momentum", type=float, default=0.0, help="rounds: --learning-momentum")
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10)
    a = ap.parse_args()
    if a.warmup is None:
        a.warmup = 5 if a.step == "kernel" else 2
    {"kernel": kernel, "rounds": rounds}[a.step](a)


if __name__ == "__main__":
    main()
