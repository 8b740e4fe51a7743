"""Probe of the MSE weight observer (`weight_observer: mse`), both observers side by side in one run on one box:

  1. cost: the first forward of full-size ConvTasNet and HTDemucs with each observer (device events; a throw-away model of the same kind
     runs first, so code-object loading and allocator growth are not in the figure), and the observer launches alone;
  2. effect: the full-size ConvTasNet convergence stream (tests/test_gpu_converge.py: never-repeating separable mixtures, keyed
     Gaussian weights) at W4A8 and W2A8 from the same seed with each observer, SI-SDR window means.

  python tools/wq_mse_probe.py [--steps 150] [--skip-train] > profiles/wq_mse_probe.txt

No threshold is attached to either number."""
import argparse
import copy
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fqss_amd import kernels as K  # noqa: E402
from fqss_amd.data import synth_batch  # noqa: E402
from fqss_amd.quantization.qat.models.load_model import create_model, quantize_model  # noqa: E402
from fqss_amd.quantization.qat.qat_utils import weight_quant_report, weight_quantizer_pairs  # noqa: E402
from fqss_amd.runtime import KDTrainStep  # noqa: E402
from fqss_amd.smoke import QCFG  # noqa: E402
from tests.helpers_cfg1 import cfg1_fill  # noqa: E402
from tests.test_gpu_converge import _run_stream  # noqa: E402

OBSERVERS = ("minmax", "mse")


def qcfg(n_bits, observer):
    return dict(QCFG, weight_n_bits=n_bits, weight_observer=observer)


def build(name, n_bits, observer):
    if name == "ConvTasNet":
        model = create_model({"name": "ConvTasNet", "n_src": 2, "kernel_size": 16, "stride": 8})
    else:
        from fqss_amd.quantization.qat.models.htdemucsq import HTDemucsQ
        model = HTDemucsQ(sources=["drums", "bass", "other", "vocals"], bottom_channels=512, segment=2.0)
    cfg1_fill(model, "S.")
    fmodel = copy.deepcopy(model)
    return quantize_model(model, qcfg(n_bits, observer)).cuda().train(), fmodel.cuda().eval()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def first_forward(name, n_bits):
    x = synth_batch(2, 8000, seed=1, device="cuda")[0] if name == "ConvTasNet" else \
        (torch.randn(1, 2, 2 * 44100, generator=torch.Generator().manual_seed(1)) * 0.1).cuda()
    print(f"\n{name}, W{n_bits}A8, first forward (weight observers run inside it)")
    for observer in OBSERVERS:
        ms = []
        for rep in range(3):                      # rep 0 is the throw-away model
            model, _ = build(name, n_bits, observer)
            with torch.no_grad():
                ms.append(timed(lambda: model(x)))
        pairs = weight_quantizer_pairs(model)

        def observers_alone():
            for wqm, w, _ in pairs:
                lo, hi = torch.empty_like(wqm.min_range.data), torch.empty_like(wqm.max_range.data)
                if observer == "mse":
                    K.wq_observe_mse(w.detach(), wqm.axis, lo, hi, wqm.n_bits)
                else:
                    K.wq_observe(w.detach(), wqm.axis, lo, hi)
        observers_alone()
        alone = min(timed(observers_alone) for _ in range(3))
        rows = weight_quant_report(model)
        err = sum(10.0 ** (-r["sqnr_db"] / 10.0) for r in rows) / len(rows)
        print(f"  {observer:7s} first forward {ms[1]:9.3f} / {ms[2]:9.3f} ms   its {len(pairs)} observer launches alone {alone:8.3f} ms   "
              f"mean per-weight noise-to-signal {10.0 * np.log10(err):7.2f} dB", flush=True)


def train_streams(steps):
    gl = np.load(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "cfg1_train_long.npz"))
    B, T, seed0 = int(gl["batch"]), int(gl["samples"]), int(gl["seed0"])
    wins = [(a, min(a + 25, steps)) for a in range(0, steps, 25)]
    print(f"\nfull-size ConvTasNet, convergence stream (B = {B}, T = {T}, seed {seed0}), {steps} steps, lr 1e-3; SI-SDR dB, window means")
    print(" " * 16 + "".join(f"  {a:3d}-{b:3d}" for a, b in wins))
    for n_bits in (4, 2):
        for observer in OBSERVERS:
            torch.manual_seed(0)
            model, fmodel = build("ConvTasNet", n_bits, observer)
            cfg1_fill(fmodel, "T.")
            step = KDTrainStep(model, fmodel, kd_lambda=0.1, lr=1e-3, clip=5.0)
            sisdr, _ = _run_stream(step, steps, B, T, seed0)
            print(f"W{n_bits}A8 {observer:7s}  " + "".join(f"  {float(sisdr[a:b].mean()):7.3f}" for a, b in wins), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--steps", type=int, default=150)
    p.add_argument("--skip-train", action="store_true")
    a = p.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    print(f"# tools/wq_mse_probe.py on {torch.cuda.get_device_name(0)}")
    for name in ("ConvTasNet", "HTDemucs"):
        first_forward(name, 4)
    if not a.skip_train:
        train_streams(a.steps)


if __name__ == "__main__":
    main()
