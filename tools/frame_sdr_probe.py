#!/usr/bin/env python3
"""Probe of the frame-wise SDR kernels (fqss_frame_sdr, csrc/track_eval.hip): one `kernels.frame_sdr` call on a 240 s stereo track of
4 sources at 44.1 kHz in 1 s windows, beside the same quantity from stock torch device operations (`unfold`, `sum`, `nanmedian` in
fp64), in one run: device events after warm-up, the median of 20 alternating repeats.

  python tools/frame_sdr_probe.py [--seconds 240] [--win-s 1.0] [--hop-s 1.0]
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/frame_sdr_probe.py --kernel-only      (per-kernel times)

No threshold is attached to any number."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fqss_amd import kernels as K  # noqa: E402


def torch_frame_sdr(est, ref, win, hop):
    """the statement of include/fqss.h in torch device operations, fp64"""
    r, e = ref.double().unfold(-1, win, hop), est.double().unfold(-1, win, hop)              # [S, C, W, win]
    num, den = (r * r).sum((1, 3)), ((r - e) ** 2).sum((1, 3))
    valid = ((r != 0).any(3).any(1) & (e != 0).any(3).any(1)).all(0)
    frames = torch.where(valid[None], 10.0 * torch.log10(num / den), torch.full_like(num, float("nan")))
    # torch.nanmedian takes the lower of two middle values: the mean of the two is the quantile form
    return torch.nanquantile(frames, 0.5, dim=1), frames


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--seconds", type=float, default=240.0)
    p.add_argument("--win-s", type=float, default=1.0)
    p.add_argument("--hop-s", type=float, default=None)
    p.add_argument("--kernel-only", action="store_true", help="for a kernel trace: no torch operations")
    a = p.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    fs, S, C = 44100, 4, 2
    L, win = int(fs * a.seconds), int(fs * a.win_s)
    hop = win if a.hop_s is None else int(fs * a.hop_s)
    g = torch.Generator("cuda").manual_seed(0)
    ref = torch.randn(S, C, L, device="cuda", generator=g) * 0.1
    est = ref + 0.03 * torch.randn(S, C, L, device="cuda", generator=g)
    ref[1, :, 5 * hop:5 * hop + win] = 0.0                             # one window that a silent stem voids
    print(f"# tools/frame_sdr_probe.py on {torch.cuda.get_device_name(0)}: S = {S}, C = {C}, L = {L} ({a.seconds:g} s at {fs} Hz), "
          f"win = {win}, hop = {hop}, W = {(L - win) // hop + 1}")
    ours = lambda: K.frame_sdr(est, ref, win, hop)
    med, frames = ours()
    print(f"med = {med.tolist()}  ({int(frames[0].isnan().sum())} invalid windows)")
    if a.kernel_only:
        for _ in range(20):
            ours()
        torch.cuda.synchronize()
        return
    stock = lambda: torch_frame_sdr(est, ref, win, hop)
    med_t, frames_t = stock()
    print(f"max |med - torch| = {(med - med_t).abs().max().item():.3g} dB, max |frames - torch| = "
          f"{(frames - frames_t).abs().nan_to_num(0.0).max().item():.3g} dB")
    for _ in range(5):
        ours(), stock()
    ms = np.array([(timed(ours), timed(stock)) for _ in range(20)])   # alternating repeats
    for name, col in (("kernels.frame_sdr", ms[:, 0]), ("torch unfold/sum/nanquantile", ms[:, 1])):
        print(f"{name:<30} median {np.median(col):8.3f} ms   min {col.min():8.3f} ms")


if __name__ == "__main__":
    main()
