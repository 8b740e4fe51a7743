#!/usr/bin/env python3
"""Golden vectors for LSTMQ_static (`lstm_quant: static`), generated from the REAL reference layer (qat_layers.py:741-862).

Runs ONLY in the build container, on the CPU (imports the reference through tools/ref_shim.py); writes the data-only fixture
tests/golden/lstmq_static.npz:

  keys / shapes         the reference's state_dict key list and shapes for nn.LSTM(16, 8, 1, bidirectional=True)
  q8.* , q24.*          QUANTIZING cases (H = 8: S = 6, B = 3 with backward; H = 24: S = 3, B = 3 forward only): weights, biases and
                        calibrated (then tightened: both clip branches are exercised) ranges under `<case>.sd.<key>`, the input, per
                        processed step and direction the carried (h, c) going in and coming out ([S, 2, B, H]: step k is time k in the
                        forward direction, time S-1-k in the reverse direction), the layer output; for q8 after backward on a recorded
                        gout the input gradient and every parameter gradient (`<case>.grad.<name>`; the 46 used range gradients among
                        them, `activation_fake_quantize_mul2_r` has none: it is never called)
  cal.*                 CALIBRATION case (H = 8, S = 56, B = 2, observer on): the first forward of a fresh module -- every quantizer's
                        ranges and n_iter afterwards, and the output

The quantizing cases are also run in fp64 (module.double()): the seed below is the first one for which the fp32 and the fp64 reference
runs agree within the index-agreement cap the GPU tests apply (every bin index within 1, at most 2e-3 of them different) on every
recorded h, c and output -- the cap is then a property of the fixture, not a measurement of the code under test.

Usage:  python tools/make_goldens_lstmq.py [--search N]
"""
import argparse
import copy
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as MG  # noqa: E402  (installs the import shim, pins torch to one thread)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from quantization.qat import qat_layers as RL  # noqa: E402
from quantization.qat import qat_quant as RQ  # noqa: E402
from quantization.qat.models.load_model import enable_observer  # noqa: E402

npy, keyed_randn = MG.npy, MG.keyed_randn
P = {'gradient_based': True, 'weight_quant': True, 'act_quant': True, 'act_n_bits': 8, 'weight_n_bits': 8}
SEED = 0            # chosen by --search (printed with the cap it met); committed
CAP_FRAC, CAP_MAX = 2e-3, 1
I_DIM = 16
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "lstmq_static.npz")


def build(seed, H):
    layer = RL.LSTMQ_static(nn.LSTM(I_DIM, H, 1, bidirectional=True), **P)
    with torch.no_grad():
        for k, p in layer.named_parameters():
            if k.endswith("min_range") or k.endswith("max_range"):
                continue
            p.copy_(keyed_randn(f"lstmq.{seed}.{H}.{k}", tuple(p.shape), 0.1 if p.dim() == 1 else 1.2 / np.sqrt(p.shape[1])))
    return layer.train()


def step_quantizers(layer):
    return {k: m for k, m in layer.named_children() if isinstance(m, RQ.GradientActivationFakeQuantize)}


def record(layer, x, S):
    """one forward with hooks on the quantizers whose outputs ARE the carried state: mul2 (both directions, forward's call first),
    add1 / add1_r -> y, h_out [S, 2, B, H], c_out"""
    hs, cf, cr = [], [], []
    hooks = [layer.activation_fake_quantize_mul2.register_forward_hook(lambda m, i, o: hs.append(o.detach().clone())),
             layer.activation_fake_quantize_add1.register_forward_hook(lambda m, i, o: cf.append(o.detach().clone())),
             layer.activation_fake_quantize_add1_r.register_forward_hook(lambda m, i, o: cr.append(o.detach().clone()))]
    y = layer(x)[0]
    for h in hooks:
        h.remove()
    assert len(hs) == 2 * S and len(cf) == S and len(cr) == S
    h_out = torch.stack([torch.stack([hs[2 * k], hs[2 * k + 1]]) for k in range(S)])
    c_out = torch.stack([torch.stack([cf[k], cr[k]]) for k in range(S)])
    return y, h_out, c_out


def idx_stats(a, b, lo, hi):
    delta = (hi - lo) / 255.0
    ia, ib = np.rint((a - lo) / delta), np.rint((b - lo) / delta)
    return float(np.mean(ia != ib)), float(np.abs(ia - ib).max())


def quantizing_case(seed, H, S, B, backward):
    layer = build(seed, H)
    enable_observer(layer, True)
    with torch.no_grad():       # 54 observed time steps (> 50: every step quantizer leaves its observer), the weight observers' one call
        for i in range(-(-54 // S)):
            layer(keyed_randn(f"lstmq.{seed}.{H}.cal{i}", (S, B, I_DIM)))
    enable_observer(layer, False)
    with torch.no_grad():       # tightened about the centre: values clip at both ends
        for m in step_quantizers(layer).values():
            lo, hi = float(m.min_range), float(m.max_range)
            m.min_range.fill_((lo + hi) / 2 - 0.93 * (hi - lo) / 2)
            m.max_range.fill_((lo + hi) / 2 + 0.93 * (hi - lo) / 2)
    x = keyed_randn(f"lstmq.{seed}.{H}.x", (S, B, I_DIM)).requires_grad_(True)
    y, h_out, c_out = record(layer, x, S)
    d = {"x": npy(x), "out": npy(y), "h_out": npy(h_out), "c_out": npy(c_out)}
    zero = torch.zeros(1, 2, B, H)
    d["h_in"] = npy(torch.cat([zero, h_out[:-1]]))
    d["c_in"] = npy(torch.cat([zero, c_out[:-1]]))
    for k, v in layer.state_dict().items():
        d["sd." + k] = npy(v)
    if backward:
        gout = keyed_randn(f"lstmq.{seed}.{H}.gout", tuple(y.shape))
        y.backward(gout)
        d["gout"], d["gin"] = npy(gout), npy(x.grad)
        for k, p in layer.named_parameters():
            if p.grad is not None:
                d["grad." + k] = npy(p.grad)
        assert "grad.activation_fake_quantize_mul2_r.min_range" not in d
    # the same run in fp64, on the fp32 run's fake-quantized weights: the symmetric weight grid puts each channel's extreme element on
    # an exact tie (|w| / delta = 127.5), which fp32 and fp64 break differently -- a property of the weight quantizer (bit-exact here,
    # tests/test_gpu_fq.py), not of the recurrence this fixture is about
    l64 = copy.deepcopy(layer)
    with torch.no_grad():
        for name, wq in layer.weight_quantizers_dict.items():
            getattr(l64.lstm, name).copy_(wq(getattr(layer.lstm, name)))
            l64.weight_quantizers_dict[name] = nn.Identity()
    l64 = l64.double()
    with torch.no_grad():
        y64, h64, c64 = record(l64, x.detach().double(), S)
    sd = layer.state_dict()
    rng = lambda q: (float(sd[q + ".min_range"]), float(sd[q + ".max_range"]))
    worst = (0.0, 0.0)
    checks = [(d["out"], npy(y64), rng("activation_fake_quantize")), (d["h_out"], npy(h64), rng("activation_fake_quantize_mul2")),
              (d["c_out"][:, 0], npy(c64)[:, 0], rng("activation_fake_quantize_add1")),
              (d["c_out"][:, 1], npy(c64)[:, 1], rng("activation_fake_quantize_add1_r"))]
    for a, b, (lo, hi) in checks:
        frac, dmax = idx_stats(a, b.astype(np.float64), lo, hi)
        worst = (max(worst[0], frac), max(worst[1], dmax))
    return d, worst


def calibration_case(seed, H=8, S=56, B=2):
    layer = build(seed, H)
    enable_observer(layer, True)
    x = keyed_randn(f"lstmq.{seed}.cal.x", (S, B, I_DIM))
    with torch.no_grad():
        y = layer(x)[0]
    d = {"x": npy(x), "out": npy(y)}
    for k, v in layer.state_dict().items():
        d["sd." + k] = npy(v)
    names = sorted(step_quantizers(layer))
    d["quantizers"] = np.array(names)
    d["n_iter"] = np.array([getattr(layer, n).n_iter for n in names], dtype=np.int64)
    assert layer.activation_fake_quantize_mul2_r.n_iter == 0 and layer.activation_fake_quantize_mul2.n_iter == 50
    return d


def all_cases(seed):
    out, worst = {}, (0.0, 0.0)
    for name, H, S, B, bwd in (("q8", 8, 6, 3, True), ("q24", 24, 3, 3, False)):
        d, w = quantizing_case(seed, H, S, B, bwd)
        out.update({f"{name}.{k}": v for k, v in d.items()})
        worst = (max(worst[0], w[0]), max(worst[1], w[1]))
    return out, worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--search", type=int, default=0, help="try seeds 0..N-1 and print the first that meets the cap")
    a = ap.parse_args()
    if a.search:
        for seed in range(a.search):
            _, (frac, dmax) = all_cases(seed)
            print(f"seed {seed}: fp32 vs fp64 reference, worst differing fraction {frac:.2e}, worst index distance {dmax:.0f}")
            if frac <= CAP_FRAC and dmax <= CAP_MAX:
                print(f"seed {seed} meets the cap (fraction <= {CAP_FRAC}, distance <= {CAP_MAX}): commit it as SEED")
                return
        raise SystemExit("no seed met the cap")
    out, (frac, dmax) = all_cases(SEED)
    print(f"seed {SEED}: fp32 vs fp64 reference, worst differing fraction {frac:.2e}, worst index distance {dmax:.0f} "
          f"(cap: fraction <= {CAP_FRAC}, distance <= {CAP_MAX})")
    assert frac <= CAP_FRAC and dmax <= CAP_MAX, "SEED no longer meets the cap: run --search"
    out.update({f"cal.{k}": v for k, v in calibration_case(SEED).items()})
    ref = RL.LSTMQ_static(nn.LSTM(16, 8, 1, bidirectional=True), **P).state_dict()
    out["keys"] = np.array(list(ref))
    out["shapes"] = np.array([",".join(str(s) for s in v.shape) for v in ref.values()])
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
