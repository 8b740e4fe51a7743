"""Probe of the histogram-MSE activation observer (`act_observer: mse`), everything in one run on one box (device events, median of 20):

  1. k_aq_hist on a full-size activation (8 x 512 x 3999 fp32), Gaussian and post-ReLU, against a plain copy of the same tensor;
  2. merge + search of one quantizer (fqss_aq_mse_search) at M about 3 000 and at the cap (M = 65 536);
  3. full-size ConvTasNet: 50 observing forwards with mse against minmax, and the 50th forward (the one-off search of every quantizer) alone;
  4. the full-size ConvTasNet convergence stream of tools/converge_probe.py (that tool takes no observer option; the same
     tests.test_gpu_converge._run_stream on the same cfg1 weights) with each observer at W8A8 and W4A8, SI-SDR window means.

  python tools/aq_mse_probe.py [--steps 150] [--skip-train] > profiles/aq_mse_probe.txt

No threshold is attached to any number."""
import argparse
import copy
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fqss_amd import kernels as K  # noqa: E402
from fqss_amd.data import synth_batch  # noqa: E402
from fqss_amd.quantization.qat import qat_quant as QQ  # noqa: E402
from fqss_amd.quantization.qat.models.load_model import create_model, quantize_model  # noqa: E402
from fqss_amd.runtime import KDTrainStep  # noqa: E402
from fqss_amd.smoke import QCFG  # noqa: E402
from tests.helpers_cfg1 import cfg1_fill  # noqa: E402

OBSERVERS = ("minmax", "mse")


def median_ms(fn, reps=20):
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def hist_probe():
    print("\n1. k_aq_hist, 8 x 512 x 3999 fp32 (65.5 MB)")
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(8, 512, 3999, device="cuda", generator=g)
    y = torch.empty_like(x)
    nbytes = x.numel() * 4
    ms = median_ms(lambda: y.copy_(x))
    print(f"  plain copy                 {ms:8.4f} ms   {nbytes / ms / 1e6:8.1f} GB/s read (+ as much written)")
    for name, t in (("gaussian", x), ("post-ReLU", torch.relu(x))):
        obs = torch.tensor([-1, 0], dtype=torch.int32, device="cuda")
        h, r = torch.zeros(K.AQ_HIST_BINS, dtype=torch.int32, device="cuda"), torch.zeros(2, device="cuda")

        def run():
            K.minmax(t, obs)
            K.aq_hist(t, obs, h, r)
        both = median_ms(run)
        mm = median_ms(lambda: K.minmax(t, obs))
        K.obs_reset(obs)
        print(f"  {name:10s} minmax + hist {both:8.4f} ms, minmax alone {mm:8.4f} ms -> hist {both - mm:8.4f} ms   "
              f"{nbytes / (both - mm) / 1e6:8.1f} GB/s read")


def search_probe():
    print("\n2. fqss_aq_mse_search (prep + merge + 10 000 candidates + argmin), one quantizer, 50 rows")
    g = np.random.default_rng(0)
    for name, scale0 in (("M about 3 000", 1.0), ("the cap", 1e-3)):
        hs, rs = [], []
        for t in range(50):
            x = (g.standard_normal(4096) * (scale0 if t == 0 else 1.0 + 0.1 * t)).astype(np.float32)
            c, _ = np.histogram(x.astype(np.float64), K.AQ_HIST_BINS)
            hs.append(c)
            rs.append((x.min(), x.max()))
        h = torch.from_numpy(np.stack(hs).astype(np.int32)).cuda()
        r = torch.tensor(rs, dtype=torch.float32).cuda()
        qmin, qmax = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
        res = K.aq_mse_search(h, r, qmin, qmax, want=True)
        ms = median_ms(lambda: K.aq_mse_search(h, r, qmin, qmax))
        print(f"  {name:14s} M = {res.M:6d}   {ms:9.4f} ms   (i, j) = {tuple(res.ij.tolist())}")


def build(observer, n_bits=8):
    model = create_model({"name": "ConvTasNet", "n_src": 2, "kernel_size": 16, "stride": 8})
    cfg1_fill(model, "S.")
    fmodel = copy.deepcopy(model)
    return quantize_model(model, dict(QCFG, weight_n_bits=n_bits, act_observer=observer)).cuda().train(), fmodel.cuda().eval()


def forward_probe():
    print("\n3. full-size ConvTasNet, B = 8, 32 000 samples: the 50 observing forwards (no_grad), device events around all of them")
    x = synth_batch(8, 32000, seed=1, device="cuda")[0]
    for observer in OBSERVERS:
        for rep in range(2):                      # rep 0 is the throw-away model
            model, _ = build(observer)
            a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            with torch.no_grad():
                model(x)
                torch.cuda.synchronize()
                a.record()
                for _ in range(48):
                    model(x)
                b.record()
                model(x)                          # call 50: with mse, the search of every quantizer
                c.record()
            torch.cuda.synchronize()
        n = sum(isinstance(m, QQ.GradientActivationFakeQuantize) and m.n_iter == 50 for m in model.modules())
        print(f"  {observer:7s} forwards 2-49: {a.elapsed_time(b) / 48:8.3f} ms each   forward 50: {b.elapsed_time(c):9.3f} ms   "
              f"({n} activation quantizers)", flush=True)


def train_streams(steps):
    from tests.test_gpu_converge import _run_stream
    gl = np.load(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "cfg1_train_long.npz"))
    B, T, seed0 = int(gl["batch"]), int(gl["samples"]), int(gl["seed0"])
    wins = [(a, min(a + 25, steps)) for a in range(0, steps, 25)]
    print(f"\n4. full-size ConvTasNet, convergence stream (B = {B}, T = {T}, seed {seed0}), {steps} steps, lr 1e-3; SI-SDR dB, window means")
    print(" " * 16 + "".join(f"  {a:3d}-{b:3d}" for a, b in wins))
    for n_bits in (8, 4):
        for observer in OBSERVERS:
            torch.manual_seed(0)
            model, fmodel = build(observer, n_bits)
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
    print("# tools/aq_mse_probe.py")
    hist_probe()
    search_probe()
    forward_probe()
    if not a.skip_train:
        train_streams(a.steps)


if __name__ == "__main__":
    main()
