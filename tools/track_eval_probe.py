#!/usr/bin/env python3
"""Time of the separation of one stereo track as val.py's nSDR mode runs it (GPU box): a full-size quantized HTDemucsQ, 60 s of
synthetic stereo at 44.1 kHz, segment 343980, overlap 0.25 (11 chunks), normalised by kernels.track_stats and scored by kernels.nsdr
-- chunk by chunk (the normalisation as tensor operations) against chunk_batch=G (the normalisation inside fqss_chunk_gather_mc /
fqss_infer_ola_chunks).  Every variant is warmed up first; then the variants take turns, each call timed with device events,
and the median of the repeats is reported with the quartiles.  The chunk-by-chunk path of the same run is the yardstick.

  python tools/track_eval_probe.py [--repeats 5] [--batches 2,4] [--seconds 60] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fqss_amd import kernels as K
from fqss_amd.process import calc_nsdr, model_infer
from fqss_amd.quantization.qat.models.load_model import create_model, enable_observer, quantize_model

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--batches", default="2,4")
ap.add_argument("--seconds", type=float, default=60.0)
ap.add_argument("--segment", type=int, default=343980)
ap.add_argument("--overlap", type=float, default=0.25)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "track_eval_probe measures on a ROCm device"

QCFG = dict(qat=True, gradient_based=True, weight_quant=True, weight_n_bits=8, act_quant=True, act_n_bits=8, in_quant=False, in_act_n_bits=8,
            out_quant=True, out_act_n_bits=8, n_splitter=2, n_combiner=2, observer=True)
torch.manual_seed(0)
m = quantize_model(create_model({"name": "HTDemucs"}), dict(QCFG)).cuda().train()
L = int(args.seconds * 44100)
track = torch.randn(len(m.sources), 2, L, device="cuda") * 0.1         # the stems; their sum is the mixture
mix = track.sum(0)
with torch.no_grad():
    for i in range(3):                      # the observers need ranges before eval mode quantizes with them
        m(mix[None, :, i * args.segment:(i + 1) * args.segment].contiguous())
enable_observer(m, False)
m.eval()
variants = [None] + [int(b) for b in args.batches.split(",") if b]


def call(G):
    stats = K.track_stats(mix)
    if G is None:
        sep = model_infer(m, (mix - stats[0]) / stats[1], segment=args.segment, overlap=args.overlap) * stats[1] + stats[0]
    else:
        sep = model_infer(m, mix, segment=args.segment, overlap=args.overlap, chunk_batch=G, stats=stats)
    return calc_nsdr(track, sep)


outs = {G: call(G).clone() for G in variants}          # warm-up
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
res = {"track_s": args.seconds, "segment": args.segment, "overlap": args.overlap,
       "chunks": len(range(0, L, int((1 - args.overlap) * args.segment))), "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
       "variants": []}
for G in variants:
    t = sorted(times[G])
    q = statistics.quantiles(t, n=4) if len(t) >= 2 else [t[0]] * 3
    diff = (outs[G] - outs[None]).abs().max().item()
    res["variants"].append({"chunk_batch": G, "median_ms": statistics.median(t), "q1_ms": q[0], "q3_ms": q[2], "min_ms": t[0],
                            "max_abs_nsdr_diff_db": diff})
    print(f"chunk_batch {str(G):>4}: median {statistics.median(t):9.3f} ms  (q1 {q[0]:.3f}, q3 {q[2]:.3f}, min {t[0]:.3f})  "
          f"nSDR {[round(v, 3) for v in outs[G].tolist()]}, max |diff to chunk by chunk| {diff:.3e} dB")
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
