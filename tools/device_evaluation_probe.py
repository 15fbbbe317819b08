#!/usr/bin/env python
"""Device-evaluation probe (measurement tool): what niidmix::linear_eval_rows costs on one GPU
against its yardsticks, at the shapes
    a   1000 jobs, one shared set of 10 000 samples, K 784,  C 10   (every node on the test set)
    b   1000 jobs, a 45-sample train segment each,   K 784,  C 10   (Logger.log_train_accuracy)
    c   1000 jobs, one shared set of 1000 samples,   K 1023, C 1024 (P = 2^20)

  kernel   device-event times, the candidates alternating within every repetition:
             eval    the op (k_lin_eval + k_lin_eval_sum)
             torch   the same result from torch ops on the device (matmul, log_softmax, argmax,
                     sum), chunked over jobs to fit
             copy    niidmix_stream_copy_f32 over the bytes the call must read (the listed rows
                     of theta, the samples and the labels once)
           then the CPU loop at torch.get_num_threads() threads: model.forward + nll_loss + argmax
           over in-memory batches of 100, timed on --cpu-nodes nodes and scaled to the job count.
           Medians with min..max; the achieved FMA rate against the 78.6 T FMA/s fp32 vector peak.
  logger   one replaced Logger.state at shape a: train (45 samples each), test and valid
           (10 000 each) events of 1000 nodes, host clock around the call (it ends in D2H copies).

    python tools/device_evaluation_probe.py kernel --shape a [--warmup 5] [--reps 20]
    python tools/device_evaluation_probe.py logger
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
sys.path[:0] = [REPO, os.path.join(REPO, "non-iid-topology-simulator_amd")]

# jobs, samples per job, shared segment, K, C
SHAPES = {"a": (1000, 10000, True, 784, 10), "b": (1000, 45, False, 784, 10),
          "c": (1000, 1000, True, 1023, 1024)}
PEAK_FMA = 78.6e12


def _stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def kernel(a):
    import torch
    import torch.nn.functional as F
    from niidmix import _lib, ops, train  # noqa: F401
    n, m, shared, k, c = SHAPES[a.shape]
    n = a.jobs or n
    dev = torch.device("cuda:0")
    p = c * k + c
    ld = train.padded_ld(p)
    gen = torch.Generator(device=dev).manual_seed(1)
    s = m if shared else n * m
    theta = torch.zeros(n, ld, device=dev)
    theta[:, :p] = (torch.rand(n, p, device=dev, generator=gen) - 0.5) * (2 / k ** 0.5)
    data = torch.rand(s, k, device=dev, generator=gen)
    labels = torch.randint(0, c, (s,), device=dev, generator=gen).to(torch.int32)
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    start = torch.zeros(n, dtype=torch.int32, device=dev) if shared else \
        (torch.arange(n, dtype=torch.int32, device=dev) * m)
    length = torch.full((n,), m, dtype=torch.int32, device=dev)
    loss = torch.empty(n, dtype=torch.float64, device=dev)
    correct = torch.empty(n, dtype=torch.int32, device=dev)
    th = theta[:, :p]

    def eval_call():
        ops.linear_eval_rows(th, data, labels, rows, start, length, m, loss, correct, None, k, c)

    jc = max(1, min(n, (1 << 28) // max(1, m * c)))           # jobs per chunk: <= 1 GiB of logits
    w3, b3 = th[:, :c * k].view(n, c, k), th[:, c * k:]
    y64 = labels.long()
    t_loss = torch.empty(n, dtype=torch.float64, device=dev)
    t_correct = torch.empty(n, dtype=torch.int64, device=dev)

    def torch_call():
        for j0 in range(0, n, jc):
            j1 = min(n, j0 + jc)
            if shared:
                z = torch.matmul(data, w3[j0:j1].transpose(1, 2)) + b3[j0:j1, None, :]
                y = y64.expand(j1 - j0, m)
            else:
                x = data.view(n, m, k)[j0:j1]
                z = torch.baddbmm(b3[j0:j1, None, :], x, w3[j0:j1].transpose(1, 2))
                y = y64.view(n, m)[j0:j1]
            lp = F.log_softmax(z, 2)
            t_loss[j0:j1] = -lp.gather(2, y[..., None]).squeeze(2).double().sum(1)
            t_correct[j0:j1] = (z.argmax(2) == y).sum(1)

    nbytes = 4 * (n * p + s * k + s)
    numel = nbytes // 4 // 4 * 4
    src = torch.empty(numel, device=dev)
    dst = torch.empty(numel, device=dev)
    strm = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def copy_call():
        _lib.check(_lib.lib.niidmix_stream_copy_f32(src.data_ptr(), dst.data_ptr(), numel, strm), "copy")

    calls = [("eval", eval_call), ("torch", torch_call), ("copy", copy_call)]
    times = {name: [] for name, _ in calls}
    for rep in range(a.warmup + a.reps):
        for name, fn in calls:
            s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            fn()
            e0.record()
            e0.synchronize()
            if rep >= a.warmup:
                times[name].append(s0.elapsed_time(e0))
    out = {"probe": "device-evaluation kernel", "shape": a.shape, "jobs": n, "samples": m, "K": k,
           "C": c, "shared": shared, "lib": _lib.lib_sha16(), "reps": a.reps,
           "threads": torch.get_num_threads()}
    for name in times:
        out[name] = _stats(times[name])
    fma = n * m * k * c
    out["eval"]["fma_per_s"] = fma / (out["eval"]["median_ms"] * 1e-3)
    out["eval"]["share_of_fp32_vector_peak"] = out["eval"]["fma_per_s"] / PEAK_FMA
    out["copy"]["bytes"] = 2 * 4 * numel
    out["copy"]["tb_per_s"] = 2 * 4 * numel / (out["copy"]["median_ms"] * 1e-3) / 1e12
    # the two device results agree (another summation order)
    out["agreement"] = {
        "correct_equal": int((correct.long() == t_correct).sum()), "of": n,
        "max_rel_loss_diff": float(((loss - t_loss).abs() / t_loss.abs().clamp_min(1e-30)).max())}

    # yardstick 1: the CPU evaluation loop on a few nodes, scaled to all jobs
    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = torch.nn.Linear(k, c)

        def forward(self, x, params):
            return F.log_softmax(self.fc(x.view(-1, k)), dim=1)
    cn = min(a.cpu_nodes, n)
    xc, yc = data.cpu(), labels.long().cpu()
    models = [Net() for _ in range(cn)]
    cpu_t = []
    for rep in range(1 + a.cpu_reps):
        t0 = time.perf_counter()
        with torch.no_grad():
            for i, mdl in enumerate(models):
                lo = 0 if shared else i * m
                tot, cor = 0.0, 0
                for b0 in range(lo, lo + m, 100):
                    xb, yb = xc[b0:min(b0 + 100, lo + m)], yc[b0:min(b0 + 100, lo + m)]
                    o = mdl.forward(xb, None)
                    tot += F.nll_loss(o, yb, reduction="sum").item()
                    cor += o.argmax(1).eq(yb).sum().item()
        if rep:
            cpu_t.append((time.perf_counter() - t0) * 1e3 * n / cn)
    out["cpu_loop"] = dict(_stats(cpu_t), timed_nodes=cn, scaled_to=n)
    print(json.dumps(out), flush=True)


def logger(a):
    import torch
    import torch.nn.functional as F
    from niidmix import evaluate, logger as nl
    n, m, k, c, own = a.jobs or 1000, 10000, 784, 10, 45
    gen = torch.Generator().manual_seed(2)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = torch.nn.Linear(k, c)

        def forward(self, x, params):
            return F.log_softmax(self.fc(x.view(-1, k)), dim=1)

    def make(count):
        return torch.utils.data.TensorDataset(torch.rand(count, k, generator=gen),
                                              torch.randint(0, c, (count,), generator=gen))
    params = {"logger": {"skip-full-training": True}, "algorithm": {"device-evaluation": True}}
    import tempfile
    with tempfile.TemporaryDirectory() as rundir:
        os.mkdir(os.path.join(rundir, "events"))
        nodes = [{"rank": r, "epoch": 0, "model": Net(), "train-set": make(own),
                  "event-file": os.path.join(rundir, "events", f"{r}.jsonlines")} for r in range(n)]

        class Logger:
            pass
        lg = Logger()
        lg.params, lg.rundir = params, rundir
        lg.running_loss, lg.running_loss_count = [0.0] * n, [0] * n
        lg.global_events = os.path.join(rundir, "events", "global.jsonlines")
        evaluate.register_sets(test=make(m), valid=make(m), params=params)
        ts = []
        for rep in range(1 + a.reps):
            t0 = time.perf_counter()
            nl.device_state(lg, nodes, {"step": rep})
            torch.cuda.synchronize()
            if rep:
                ts.append((time.perf_counter() - t0) * 1e3)
    from niidmix import _lib
    print(json.dumps({"probe": "device-evaluation Logger.state", "nodes": n, "test": m, "valid": m,
                      "train_each": own, "lib": _lib.lib_sha16(), "reps": a.reps,
                      "source": evaluate.default(params).last_source, **_stats(ts)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("step", choices=["kernel", "logger"])
    ap.add_argument("--shape", choices=list(SHAPES), default="a")
    ap.add_argument("--jobs", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-nodes", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=3)
    a = ap.parse_args()
    {"kernel": kernel, "logger": logger}[a.step](a)


if __name__ == "__main__":
    main()
