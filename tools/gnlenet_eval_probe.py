#!/usr/bin/env python
"""Timings behind DESIGN §5 "GN-LeNet evaluation": niidmix::gnlenet_eval_rows (k_gnl_eval) against
niidmix::gnlenet_eval_rows_mfma (k_gnl_eval_mfma) on one GPU.

Per shape the two ops run on the same inputs, alternating in one process: --rows slab rows of
random GN-LeNet parameters, each evaluated on the same --samples samples (one job per row), device
events around each op call (the evaluation kernel and k_lin_eval_sum), --warmup repetitions, then
median, minimum and maximum of --reps.  Reported with the network's own FMAs (conv1 counted once
per output position, not per pooled window) as TFLOP/s and as a fraction of the 157.3 TFLOP/s fp32
matrix peak, the two ops' largest logit difference, and whether the matrix-core kernel's median is
below the other's (niidmix.family's routing rule reads that).

    python tools/gnlenet_eval_probe.py                     # 1 x 28 x 28 x 10 and 3 x 32 x 32 x 10

One JSON line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "non-iid-topology-simulator_amd"))
PEAK_TFLOPS = 157.3


def flops(cin, h, w, c):
    """2 x the FMAs of one forward pass, (total, conv2 + conv3)."""
    def down(v):
        return (v - 3) // 2 + 1
    hw1 = down(h) * down(w)
    hw2 = down(down(h)) * down(down(w))
    f = 64 * down(down(down(h))) * down(down(down(w)))
    mm = 2 * 800 * (32 * hw1 + 64 * hw2)
    return 2 * 32 * cin * 25 * h * w + mm + 2 * f * c, mm


def one_shape(a, shape, torch, ops):
    cin, h, w, c = shape
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(11)
    p = ops.gnlenet_sizes(cin, h, w, c)[1]
    ld = (p + 3) // 4 * 4
    theta = (0.05 * torch.randn(a.rows, ld, device=dev, generator=gen))[:, :p]
    off = 0                               # GroupNorm weights near 1, as a trained model has them
    for i, sh in enumerate(ops.gnlenet_shapes(cin, c, ops.gnlenet_sizes(cin, h, w, c)[0])):
        n = 1
        for v in sh:
            n *= v
        if i in (2, 6, 10):
            theta[:, off:off + n] += 1.0
        off += n
    data = torch.randn(a.samples, cin * h * w, device=dev, generator=gen)
    labels = torch.randint(0, c, (a.samples,), device=dev, generator=gen).to(torch.int32)
    rows = torch.arange(a.rows, dtype=torch.int32, device=dev)
    start = torch.zeros(a.rows, dtype=torch.int32, device=dev)
    length = torch.full((a.rows,), a.samples, dtype=torch.int32, device=dev)
    loss = torch.empty(a.rows, dtype=torch.float64, device=dev)
    correct = torch.empty(a.rows, dtype=torch.int32, device=dev)
    cands = [("k_gnl_eval", ops.gnlenet_eval_rows), ("k_gnl_eval_mfma", ops.gnlenet_eval_rows_mfma)]
    z = {}
    for name, op in cands:                # the outputs, once, outside the timed calls
        z[name] = torch.empty(a.rows, a.samples, c, device=dev)
        op(theta, data, labels, rows, start, length, a.samples, loss, correct, None, z[name], *shape)
    diff = float((z["k_gnl_eval"] - z["k_gnl_eval_mfma"]).abs().max())
    zmax = float(z["k_gnl_eval"].abs().max())
    del z
    times = {name: [] for name, _ in cands}
    for r in range(a.warmup + a.reps):
        for name, op in cands:
            s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            op(theta, data, labels, rows, start, length, a.samples, loss, correct, None, None, *shape)
            e0.record()
            e0.synchronize()
            if r >= a.warmup:
                times[name].append(s0.elapsed_time(e0) * 1e-3)
    total, mm = flops(*shape)
    out = {"shape": list(shape), "tile": ops.gn_mfma_tile(h, w), "flop_per_sample": total,
           "conv23_share": mm / total, "max_logit_diff": diff, "max_abs_logit": zmax}
    for name, _ in cands:
        t = times[name]
        med = statistics.median(t)
        tf = total * a.rows * a.samples / med / 1e12
        out[name] = {"median_ms": med * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3,
                     "tflops_median": tf, "fraction_of_fp32_matrix_peak": tf / PEAK_TFLOPS}
    out["mfma_over_existing"] = out["k_gnl_eval_mfma"]["median_ms"] / out["k_gnl_eval"]["median_ms"]
    out["mfma_faster"] = out["k_gnl_eval_mfma"]["median_ms"] < out["k_gnl_eval"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    from niidmix import _lib, ops
    if not torch.cuda.is_available():
        sys.exit("gnlenet_eval_probe: no GPU (a timing needs one)")
    out = {"step": "gnlenet_eval", "rows": a.rows, "samples": a.samples, "warmup": a.warmup,
           "reps": a.reps, "device": torch.cuda.get_device_name(0), "lib_sha16": _lib.lib_sha16(),
           "shapes": [one_shape(a, sh, torch, ops) for sh in ((1, 28, 28, 10), (3, 32, 32, 10))]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
