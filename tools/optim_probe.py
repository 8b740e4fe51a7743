#!/usr/bin/env python3
"""Time of the fused clip + update launch for every optimizer of the family, and of 0 / 1 / 2 EMA copies behind it, at the arena sizes
of ConvTasNet (5.13 M floats) and HTDemucs (41.5 M floats), in ONE run on one box (GPU box).  A turn of a variant is what a step
issues for it -- fqss_sumsq, the update (fqss_adam_clip or fqss_optim_clip), one fqss_ema_update_dev per copy -- timed with device
events; the variants take turns, so a busy moment on the box falls on all of them, and the median of the repeats is reported with the
quartiles.  `adam_clip` of the same run is the yardstick.  The kernels are bounded by their bytes, which the output
states per variant so that the achieved GB/s can be read off.

  python tools/optim_probe.py [--repeats 20] [--sizes 5130240,41500032] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fqss_amd import kernels as K

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--sizes", default="5130240,41500032", help="arena sizes in floats (multiples of 64)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "optim_probe measures on a ROCm device"

# name -> (entry point, optimizer arguments, EMA copies, bytes per element: read + written, t0 and the decay table included)
VARIANTS = {
    "adam_clip": ("adam", {}, 0, 32),
    "optim adam wd=0": ("optim", dict(kind="adam"), 0, 32),
    "optim adam l2": ("optim", dict(kind="adam", weight_decay=1e-3), 0, 32),
    "optim adamw": ("optim", dict(kind="adamw", weight_decay=1e-2), 0, 32),
    "optim adamw + table": ("optim", dict(kind="adamw", weight_decay=1e-2, table=True), 0, 32 + 1 / 16),
    "optim sgd": ("optim", dict(kind="sgd", weight_decay=1e-2), 0, 16),
    "optim sgd momentum": ("optim", dict(kind="sgd", weight_decay=1e-2, momentum=0.9), 0, 24),
    "optim sgd nesterov": ("optim", dict(kind="sgd", weight_decay=1e-2, momentum=0.9, nesterov=True), 0, 24),
    "adam_clip + 1 ema": ("adam", {}, 1, 32 + 12),
    "adam_clip + 2 ema": ("adam", {}, 2, 32 + 24),
}


def make(n, name):
    entry, kw, copies, _ = VARIANTS[name]
    g = torch.Generator().manual_seed(0)
    s = dict(p=torch.randn(n, generator=g).cuda(), g=(torch.randn(n, generator=g) * 0.05).cuda(), m=torch.zeros(n, device="cuda"),
             v=torch.zeros(n, device="cuda"), t0=torch.zeros(n, device="cuda", dtype=torch.int32),
             acc=torch.zeros(1, device="cuda", dtype=torch.float64), step=torch.zeros(1, device="cuda", dtype=torch.int32),
             gn=torch.zeros(1, device="cuda"), ema=[torch.zeros(n, device="cuda") for _ in range(copies)],
             count=torch.zeros(max(copies, 1), device="cuda", dtype=torch.float64))
    kw = dict(kw)
    s["table"] = torch.full((n // 64,), 1e-2, device="cuda") if kw.pop("table", False) else None
    s["entry"], s["kw"] = entry, kw
    return s


def turn(s):
    s["acc"].zero_()
    K.sumsq(s["g"], s["acc"])
    if s["entry"] == "adam":
        K.adam_clip(s["p"], s["g"], s["m"], s["v"], s["acc"], s["step"], s["gn"], 5.0, 1.0, 1e-3, t0=s["t0"])
    else:
        K.optim_clip(s["p"], s["g"], s["m"], s["v"], s["acc"], s["step"], s["gn"], 5.0, 1.0, 1e-3, t0=s["t0"], wd_slot=s["table"], **s["kw"])
    for k, e in enumerate(s["ema"]):
        K.ema_update(e, s["p"], decay=0.999, count=s["count"][k:k + 1])


res = {"repeats": args.repeats, "device": torch.cuda.get_device_name(0), "unit": "us per update (sumsq + update + EMA launches)", "sizes": []}
for n in (int(x) for x in args.sizes.split(",") if x):
    assert n % 64 == 0, "arena sizes are multiples of 64 floats"
    states = {name: make(n, name) for name in VARIANTS}
    for s in states.values():
        for _ in range(3):
            turn(s)
    torch.cuda.synchronize()
    times = {name: [] for name in VARIANTS}
    for _ in range(args.repeats):
        for name, s in states.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            turn(s)
            t1.record()
            t1.synchronize()
            times[name].append(1e3 * t0.elapsed_time(t1))
    base = statistics.median(times["adam_clip"])
    rows = []
    print(f"arena of {n} floats ({4e-6 * n:.1f} MB)")
    for name in VARIANTS:
        t = sorted(times[name])
        q = statistics.quantiles(t, n=4) if len(t) >= 2 else [t[0]] * 3
        med, bpe = statistics.median(t), VARIANTS[name][3] + 4          # + 4 B: fqss_sumsq reads the gradient once more
        rows.append({"variant": name, "median_us": med, "q1_us": q[0], "q3_us": q[2], "min_us": t[0], "vs_adam_clip": med / base,
                     "bytes_per_element": bpe, "GBps_at_median": bpe * n / med * 1e-3})
        print(f"  {name:22s} median {med:9.1f} us  (q1 {q[0]:.1f}, q3 {q[2]:.1f}, min {t[0]:.1f})  x{med / base:.3f} of adam_clip  "
              f"{bpe:.2f} B/element -> {bpe * n / med * 1e-3:.0f} GB/s")
    res["sizes"].append({"floats": n, "variants": rows})
    del states
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
