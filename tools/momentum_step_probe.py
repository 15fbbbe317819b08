#!/usr/bin/env python
"""Momentum-step rate probe (measurement tool): at the headline shape, in one process, the byte
rates of
  copy    niidmix_stream_copy_f32 over one [N, P] slab           (8 B per element)
  sgd     k_sgd_step_rows, every row stepped                      (12 B per element)
  mom     k_sgd_momentum_step_rows in steady state                (20 B per element)
  first   k_sgd_momentum_step_rows, first step (buf is not read)  (16 B per element)
timed with device events around single launches, the four alternating within every repetition
(warm-ups first, then the median, minimum and maximum of the timed repetitions), so the stream
copy and k_sgd_step_rows of the same run are the yardstick for the new kernel.

    python tools/momentum_step_probe.py [--n 1000] [--p 1048576] [--warmup 5] [--reps 20]

Prints one line per kernel and a final JSON line (rates in GB/s, the device and the library hash).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "non-iid-topology-simulator_amd")]
import torch  # noqa: E402

from niidmix import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--p", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("momentum_step_probe: no GPU (a rate is only ever measured on one)")
    dev = torch.device("cuda:0")
    n, p = a.n, a.p
    gen = torch.Generator(device=dev).manual_seed(1)
    xp = torch.randn(n, p, device=dev, generator=gen)
    xg = torch.randn(n, p, device=dev, generator=gen)
    xb = torch.zeros(n, p, device=dev)
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    strm = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lib = _lib.lib
    numel = n * p - (n * p) % 4
    neg_lr, mom = -1e-3, 0.9

    def copy():
        return lib.niidmix_stream_copy_f32(xg.data_ptr(), xb.data_ptr(), numel, strm)

    def sgd():
        return lib.niidmix_sgd_step_rows_f32(xp.data_ptr(), p, xg.data_ptr(), p, p, rows.data_ptr(),
                                             n, neg_lr, strm)

    def momentum(first):
        return lib.niidmix_sgd_momentum_step_rows_f32(xp.data_ptr(), p, xg.data_ptr(), p,
                                                      xb.data_ptr(), p, p, rows.data_ptr(), n,
                                                      neg_lr, mom, first, strm)

    # copy goes first in a repetition (it overwrites buf), `first` next (it re-seeds buf from g)
    kernels = [("copy", copy, 8), ("first", lambda: momentum(1), 16),
               ("mom", lambda: momentum(0), 20), ("sgd", sgd, 12)]
    times = {k: [] for k, _, _ in kernels}
    for rep in range(a.warmup + a.reps):
        for name, fn, _ in kernels:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            _lib.check(fn(), name)
            e.record()
            e.synchronize()
            if rep >= a.warmup:
                times[name].append(s.elapsed_time(e) * 1e-3)
    assert bool(torch.isfinite(xp[::97, ::4099]).all())
    out = {"n": n, "p": p, "warmup": a.warmup, "reps": a.reps,
           "device": torch.cuda.get_device_name(dev), "lib_sha16": _lib.lib_sha16()}
    for name, _, bpe in kernels:
        gb = n * p * bpe / 1e9
        t = times[name]
        med, lo, hi = statistics.median(t), min(t), max(t)
        out[name] = {"bytes_per_element": bpe, "median_ms": med * 1e3, "gbps_median": gb / med,
                     "gbps_min": gb / hi, "gbps_max": gb / lo}
        print(f"{name:6s} {bpe:2d} B/elem  median {med * 1e3:8.3f} ms  {gb / med:7.1f} GB/s "
              f"(spread {gb / hi:.1f} .. {gb / lo:.1f})")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
