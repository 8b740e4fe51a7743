#!/usr/bin/env python
"""Time of the loss sequence (memset + moments + final + gradient) at three sources (fqss_kd_loss_n) beside the two-source sequence
(fqss_kd_loss) of the same run, at cfg 2's loss shape: B = 8, T = 32000.

Device events around one call, both shapes warmed up, the two alternating, median of --reps (>= 20).  The three-source pass reads and
writes 1.5 x the rows of the two-source one: that ratio is the yardstick.  Prints one JSON line.

    python tools/nsrc_loss_probe.py [--reps 50] [--out FILE]

Per-kernel times come from a kernel trace of this script run on its own (--reps 20 keeps the trace short)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from fqss_amd import _lib, data, kernels as K  # noqa: E402


def operands(S, B, T):
    _, s = data.synth_batch(B, T, seed=3, n_src=S)
    g = torch.Generator().manual_seed(5)
    e = s + 0.3 * 0.05 * torch.randn(B, S, T, generator=g)
    f = s + 0.2 * 0.05 * torch.randn(B, S, T, generator=g)
    return e.cuda(), f.cuda(), s.cuda()


def launcher(S, e, f, s):
    """the entry point on preallocated buffers: nothing but the four enqueues sits between the two events"""
    B, _, T = e.shape
    stats = torch.empty(B, 32 if S == 2 else K.KD_STATS_STRIDE_N, device="cuda", dtype=torch.float64)
    out, w, sisdr, gest = torch.empty(4, device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, device="cuda"), torch.empty_like(e)
    st = torch.cuda.current_stream().cuda_stream
    p = [t.data_ptr() for t in (e, f, s, stats, out, w, sisdr, gest)]
    if S == 2:
        return lambda: _lib.call("fqss_kd_loss", p[0], p[1], p[2], B, T, 0.1, *p[3:], st)
    return lambda: _lib.call("fqss_kd_loss_n", p[0], p[1], p[2], B, S, T, 0.1, 0, 0, 0.0, *p[3:], st)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--samples", type=int, default=32000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20
    ops = {S: operands(S, a.batch, a.samples) for S in (2, 3)}
    run = {S: launcher(S, *ops[S]) for S in (2, 3)}
    for _ in range(10):
        for S in (2, 3):
            run[S]()
    torch.cuda.synchronize()
    times = {2: [], 3: []}
    for _ in range(a.reps):
        for S in (2, 3):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            run[S]()
            t1.record()
            t1.synchronize()
            times[S].append(1e3 * t0.elapsed_time(t1))
    med = {S: statistics.median(v) for S, v in times.items()}
    rec = {"shape": [a.batch, a.samples], "reps": a.reps, "kd_loss_2src_us": round(med[2], 2), "kd_loss_n_3src_us": round(med[3], 2),
           "ratio": round(med[3] / med[2], 3), "ratio_by_rows": 1.5,
           "min_us": {"2": round(min(times[2]), 2), "3": round(min(times[3]), 2)}}
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
