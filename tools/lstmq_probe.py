"""The quantized LSTM recurrence (fqss_lstmq_fwd / fqss_lstmq_bwd, LSTMQ_static) against the float one it extends (fqss_lstm_fwd /
fqss_lstm_bwd_b4, LSTMQ) at the cfg-3 layer shapes: H = 128, S = 250 steps x 66 sequences (intra-chunk) and S = 66 x 250 (inter-chunk).
One process; every call captured into a graph and warmed; device events around each replay; the four calls alternate and the median of
`reps` repeats is printed, with the ratios.  python tools/lstmq_probe.py [reps]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fqss_amd import kernels as K  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
torch.manual_seed(0)
dev = "cuda"
H = 128
# plausible calibrated ranges in the order of K.LSTMQ_SITES: pre-activations, the three sigmoids, the two tanh, the products, the cell
SPAN = dict(ih=(-3.0, 3.0), hh=(-2.0, 2.0), add0=(-4.0, 4.0), sig0=(0.02, 0.98), sig1=(0.02, 0.98), sig2=(0.02, 0.98), tanh0=(-0.97, 0.97),
            tanh1=(-0.95, 0.95), mul0=(-1.5, 1.5), mul1=(-0.9, 0.9), add1=(-2.0, 2.0), mul2=(-0.9, 0.9))


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    return g


for S, B in ((250, 66), (66, 250)):
    pre = torch.randn(S, B, 8 * H, device=dev) * 0.5
    whh = torch.randn(2, 4 * H, H, device=dev) / H ** 0.5
    bhh = torch.randn(2, 4 * H, device=dev) * 0.1
    gout = torch.randn(S, B, 2 * H, device=dev)
    ranges = [tuple(torch.tensor([v], device=dev) for v in SPAN[s]) for _ in range(2) for s in K.LSTMQ_SITES]
    gaccs = [torch.zeros(K.GACC_DOUBLES, dtype=torch.float64, device=dev) for _ in range(23)] + [None]
    gb4 = [torch.zeros(4 * H, device=dev) for _ in range(4)]
    _, gsav, csav = K.lstm_fwd(pre, whh, bhh, S, B, H)
    hq, _, hsav, cqsav = K.lstmq_fwd(pre, whh, bhh, ranges, S, B, H)
    calls = {
        "fqss_lstm_fwd": lambda: K.lstm_fwd(pre, whh, bhh, S, B, H),
        "fqss_lstmq_fwd": lambda: K.lstmq_fwd(pre, whh, bhh, ranges, S, B, H),
        "fqss_lstm_bwd_b4": lambda: K.lstm_bwd(gout, whh, gsav, csav, S, B, H, gb4=gb4),
        "fqss_lstmq_bwd": lambda: K.lstmq_bwd(gout, whh, pre, hsav, cqsav, ranges, gaccs, S, B, H),
    }
    graphs = {n: graph_of(f) for n, f in calls.items()}
    times = {n: [] for n in calls}
    for _ in range(reps):
        for n, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) * 1e3)
    med = {n: statistics.median(v) for n, v in times.items()}
    lo, hi = SPAN["mul2"]           # how much of the h grid the operands exercise: distinct codes, share at a clipped end
    codes = torch.round((hq - lo) / ((hi - lo) / 255.0))
    used, clipped = int(codes.unique().numel()), float(((codes <= 0) | (codes >= 255)).float().mean())
    for n in calls:
        print(f"S {S:3d} B {B:3d} {n:18s} {med[n]:9.1f} us  ({med[n] / S:6.2f} us per step)", flush=True)
    print(f"S {S:3d} B {B:3d} quantized / float: forward {med['fqss_lstmq_fwd'] / med['fqss_lstm_fwd']:.2f}, "
          f"backward {med['fqss_lstmq_bwd'] / med['fqss_lstm_bwd_b4']:.2f}   (h: {used} of 256 codes in use, {clipped:.3f} at a clipped end)", flush=True)
