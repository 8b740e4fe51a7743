#!/usr/bin/env python3
"""Time of one micro-batch of the cfg-2 training step (full-size ConvTasNet, B = 8, T = 32000, quantizing phase, hipGraphs warmed,
teacher one batch ahead) under gradient accumulation: `KDTrainStep(accumulate=N)` for N = 1, 2, 4 in ONE run on one box (GPU box).
A turn of a variant is one whole window -- N micro-batches, the accumulate launches between the replays, one exchange-free clip + Adam
-- timed with device events and divided by N; the variants take turns, and the median of the repeats is reported with the quartiles.
The accumulate=1 leg of the same run (the one-graph replay) is the yardstick: what a micro-batch costs beyond it is the accumulate
launch (one pass over the 20.5 MB arena pair) plus the two-graph replay, minus the share of clip + Adam it no longer pays.

  python tools/accum_probe.py [--repeats 20] [--accumulate 1,2,4] [--batch 8] [--samples 32000] [--out FILE.json]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/accum_probe.py --repeats 3 --accumulate 2      (per-kernel times)"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fqss_amd.data import synth_batch
from fqss_amd.quantization.qat.qat_quant import GradientActivationFakeQuantize
from fqss_amd.runtime import KDTrainStep
from fqss_amd.smoke import build_pair

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--accumulate", default="1,2,4")
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--samples", type=int, default=32000)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "accum_probe measures on a ROCm device"

variants = [int(n) for n in args.accumulate.split(",") if n]
X = [synth_batch(args.batch, args.samples, seed=100 + 100 * i, device="cuda") for i in range(2)]      # two alternating batches


def window(step, it):
    """one window of step.accumulate micro-batches over the alternating batches; -> the next batch index"""
    for _ in range(step.accumulate):
        last[step.accumulate] = step(*X[it & 1], x_next=X[(it + 1) & 1][0])
        it += 1
    return it


steps, its, last = {}, {}, {}
for N in variants:                          # every variant: its own model pair from one seed, through the observer phase, graphs captured
    model, fmodel = build_pair("cuda", 0, n_spks=2, kernel_size=16, stride=8)
    step = KDTrainStep(model, fmodel, kd_lambda=0.1, lr=1e-3, clip=5.0, teacher_ahead=True, accumulate=N)
    it = window(step, 0)
    with torch.no_grad():
        for _ in range(49):
            model(X[0][0])
    assert all(m.n_iter >= 50 for m in model.modules() if isinstance(m, GradientActivationFakeQuantize))
    it = window(step, it)                   # an eager quantizing window: tables built, the ranges' Adam clocks started
    step.capture(*X[it & 1])
    assert (getattr(step, "_graph_all", None) is not None) == (N == 1)
    for _ in range(2):
        it = window(step, it)
    assert step.pending == 0
    steps[N], its[N] = step, it
torch.cuda.synchronize()
times = {N: [] for N in variants}
for _ in range(args.repeats):               # the variants take turns, so a busy moment on the box falls on all of them
    for N in variants:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        its[N] = window(steps[N], its[N])
        t1.record()
        t1.synchronize()
        times[N].append(t0.elapsed_time(t1) / N)
res = {"batch": args.batch, "samples": args.samples, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
       "arena_MB": 4e-6 * steps[variants[0]].arena.numel, "unit": "ms per micro-batch", "variants": []}
for N in variants:
    t = sorted(times[N])
    q = statistics.quantiles(t, n=4) if len(t) >= 2 else [t[0]] * 3
    loss = last[N]["loss"].item()
    res["variants"].append({"accumulate": N, "median_ms": statistics.median(t), "q1_ms": q[0], "q3_ms": q[2], "min_ms": t[0], "last_loss": loss})
    print(f"accumulate {N:>2}: median {statistics.median(t):8.3f} ms per micro-batch  (q1 {q[0]:.3f}, q3 {q[2]:.3f}, min {t[0]:.3f})  last loss {loss:.4f}")
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
