#!/usr/bin/env python3
"""Probe of the STOI kernels (csrc/stoi.hip): one `kernels.stoi` call on two pairs of 10 s at 8 kHz beside `kernels.sdr` of the same
pairs and `process.model_infer` of the same utterance (full ConvTasNet, whole utterance), device events after warm-up, median of 20.

  python tools/stoi_probe.py [--fs 8000] [--seconds 10]
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/stoi_probe.py --stoi-only      (per-kernel times)

No threshold is attached to any number."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fqss_amd import kernels as K  # noqa: E402
from fqss_amd import process  # noqa: E402
from fqss_amd.data import synth_batch  # noqa: E402
from fqss_amd.quantization.qat.models.load_model import create_model, enable_observer, quantize_model  # noqa: E402
from fqss_amd.smoke import QCFG  # noqa: E402


def median_ms(fn, warmup=5, runs=20):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms))


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--fs", type=int, default=8000)
    p.add_argument("--seconds", type=float, default=10.0)
    p.add_argument("--stoi-only", action="store_true", help="for a kernel trace: no model, no SDR")
    a = p.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    L = int(a.fs * a.seconds)
    mix, clean = synth_batch(1, L, seed=3, device="cuda")
    clean = clean[0]                                                   # [2, L]
    est = clean + 0.3 * torch.randn(clean.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * clean.std()
    print(f"# tools/stoi_probe.py on {torch.cuda.get_device_name(0)}: P = 2 pairs, L = {L} ({a.seconds:g} s at {a.fs} Hz)")
    d = K.stoi(est, clean, a.fs)
    print(f"d = {d.tolist()}")
    med, best = median_ms(lambda: K.stoi(est, clean, a.fs))
    print(f"kernels.stoi           median {med:8.3f} ms   min {best:8.3f} ms")
    if a.stoi_only:
        return
    med, best = median_ms(lambda: K.sdr(est, clean))
    print(f"kernels.sdr            median {med:8.3f} ms   min {best:8.3f} ms")
    torch.manual_seed(0)
    model = quantize_model(create_model({"name": "ConvTasNet", "n_src": 2, "kernel_size": 16, "stride": 8}), dict(QCFG)).cuda().train()
    with torch.no_grad():
        model(synth_batch(2, 8000, seed=1, device="cuda")[0])          # the observers' first forward
    enable_observer(model, False)
    model.eval()
    med, best = median_ms(lambda: process.model_infer(model, mix[0], n_srcs=2, device="cuda"))
    print(f"process.model_infer    median {med:8.3f} ms   min {best:8.3f} ms   (whole utterance)")


if __name__ == "__main__":
    main()
