#!/usr/bin/env python3
"""Time of `process.model_infer` on one utterance, chunk by chunk against chunk_batch=G (GPU box): the full-size quantized ConvTasNet,
10 s at 8 kHz, segment 8000, overlap 0.25 (14 chunks), with a target so that every chunk is re-ordered -- what val.py does per
utterance.  Every variant is warmed up (graphs captured) first; then the variants take turns, each call timed with device events, and
the median of the repeats is reported with the quartiles.  The serial path of the same run is the yardstick; outputs are compared.

  python tools/infer_chunk_probe.py [--repeats 20] [--batches 4,8,16] [--eager] [--seconds 10] [--out FILE.json]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/infer_chunk_probe.py --repeats 3 --batches 8      (per-kernel times)"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fqss_amd.data import synth_batch
from fqss_amd.process import model_infer
from fqss_amd.quantization.qat.models.load_model import create_model, enable_observer, quantize_model
from fqss_amd.runtime import InferRunner
from fqss_amd.smoke import QCFG

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--batches", default="4,8,16")
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--segment", type=int, default=8000)
ap.add_argument("--overlap", type=float, default=0.25)
ap.add_argument("--eager", action="store_true", help="call the module itself instead of InferRunner's graphs")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "infer_chunk_probe measures on a ROCm device"

torch.manual_seed(0)
m = quantize_model(create_model({"name": "ConvTasNet", "n_src": 2, "kernel_size": 16, "stride": 8}), dict(QCFG)).cuda().train()
L = int(args.seconds * 8000)
x, _ = synth_batch(2, 32000, seed=0, device="cuda")
with torch.no_grad():
    for _ in range(20):                     # the observers need ranges before eval mode quantizes with them
        m(x)
enable_observer(m, False)
m.eval()
mix, clean = synth_batch(1, L, seed=1, device="cuda")
mix, clean = mix.reshape(1, L).contiguous(), clean.reshape(2, L).contiguous()
model = m if args.eager else InferRunner(m)
variants = [None] + [int(b) for b in args.batches.split(",") if b]


def call(G):
    kw = {} if G is None else {"chunk_batch": G}
    return model_infer(model, mix, n_srcs=2, segment=args.segment, overlap=args.overlap, target=clean, **kw)


outs = {}
for G in variants:                          # warm-up: every shape of every variant, graphs captured
    for _ in range(2):
        outs[G] = call(G).clone()
torch.cuda.synchronize()
times = {G: [] for G in variants}
for _ in range(args.repeats):               # the variants take turns, so a busy moment on the box falls on all of them
    for G in variants:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call(G)
        t1.record()
        t1.synchronize()
        times[G].append(t0.elapsed_time(t1))
res = {"utterance_s": args.seconds, "segment": args.segment, "overlap": args.overlap, "chunks": len(range(0, L, int((1 - args.overlap) * args.segment))),
       "launch": "eager" if args.eager else "graph", "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "variants": []}
for G in variants:
    t = sorted(times[G])
    q = statistics.quantiles(t, n=4) if len(t) >= 2 else [t[0]] * 3
    diff = (outs[G] - outs[None]).abs().max().item()
    res["variants"].append({"chunk_batch": G, "median_ms": statistics.median(t), "q1_ms": q[0], "q3_ms": q[2], "min_ms": t[0],
                            "equal_to_serial": bool(torch.equal(outs[G], outs[None])), "max_abs_diff": diff})
    print(f"chunk_batch {str(G):>4}: median {statistics.median(t):8.3f} ms  (q1 {q[0]:.3f}, q3 {q[2]:.3f}, min {t[0]:.3f})  "
          f"equal to serial {res['variants'][-1]['equal_to_serial']}, max |diff| {diff:.3e}")
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
