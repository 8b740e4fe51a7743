#!/usr/bin/env python3
"""Fixtures for weight quantizers at 2 to 7 bits (`weight_n_bits`) from the REAL reference (build container only; one torch thread).

  fq_w_bits.npz      qat_quant.GradientWeightFakeQuantize (qat_quant.py:126-135, 350-381) at n_bits in {2, ..., 7}: the four shape /
                     axis cases of tools/make_goldens.py::gen_fq_w with the same range perturbation and exact-tie channel, keys
                     `n{n}.{w,g,axis,min,max,y,idx,gw,gmin,gmax}{case}`.  A case whose w / delta comes within 1e-4 of a half-integer is
                     re-drawn under another key, so the bit-exact gates on idx / y / gw never hinge on a rounding tie.
  tiny_step_w4.npz   tools/make_goldens.py::gen_tiny_step with weight_n_bits = 4 (W4A8), everything else as in QCFG: same tiny net,
                     batch, optimizer and recorded steps {1, 2, 50, 51, 52, 53}.  Kept below 1 MiB: per-layer activations of step 51 only,
                     gradients of steps 1-2 only, the full state after step 50 only (quantizer ranges after every recorded step); plus
                     `s51.loss_f64`, the step-51 forward loss from the step-50 state with model and input cast to float64 (the
                     reference's own fp32 sensitivity at that point).

    python tools/make_goldens_wbits.py [--out tests/golden]"""
import argparse
import copy
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as MG  # noqa: E402  (installs the shim, imports the reference, one torch thread)

RL, RQ, npy, keyed_randn = MG.RL, MG.RQ, MG.npy, MG.keyed_randn
BITS = (2, 3, 4, 5, 6, 7)
SHAPES = [((12, 5, 3), 0), ((6, 9, 1), 0), ((7, 1, 16), 1), ((5, 4, 16), 1)]
TIE_MARGIN = 1e-4


def _fq_w_case(n, ci, shape, axis, draw):
    """one case from the reference; None when some w / delta lies within TIE_MARGIN of a half-integer (the caller re-draws)"""
    tag = f"fq_w_bits.n{n}" + (f".r{draw}" if draw else "")
    w = keyed_randn(f"{tag}.w{ci}", shape, 0.2)
    g = keyed_randn(f"{tag}.g{ci}", shape)
    q = RQ.GradientWeightFakeQuantize(True, shape, n_bits=n, ch_out_idx=axis)
    assert torch.equal(q(w), w)          # observer call: records amax/amin, returns w unquantized
    with torch.no_grad():                # the perturbation of gen_fq_w: clipping, |min| <> |max| and one exact tie |min| == |max|
        q.min_range.mul_(0.8)
        q.max_range.mul_(0.9)
        q.min_range.view(-1)[0] = -q.max_range.view(-1)[0]
    wr = w.clone().requires_grad_(True)
    y = q(wr)
    y.backward(g)
    with torch.no_grad():
        L = 2 ** n - 1
        dl = 2 * torch.maximum(q.min_range.abs(), q.max_range.abs()) / L          # the reference's own step (fp32)
        for u in (w / dl, w.double() / dl.double()):
            if float(((u - torch.floor(u)) - 0.5).abs().min()) <= TIE_MARGIN:
                return None
        idx = torch.round(y / dl)                                                 # the code the reference's OUTPUT sits on
        assert torch.equal(dl * idx, y)
        assert torch.equal(idx, torch.clip(torch.round(w / dl), -2 ** (n - 1), 2 ** (n - 1) - 1))
        assert int(idx.min()) >= -2 ** (n - 1) and int(idx.max()) <= 2 ** (n - 1) - 1
    return {"w": npy(w), "g": npy(g), "axis": np.array(axis), "min": npy(q.min_range), "max": npy(q.max_range), "y": npy(y),
            "idx": npy(idx.to(torch.int8)), "gw": npy(wr.grad), "gmin": npy(q.min_range.grad), "gmax": npy(q.max_range.grad)}


def gen_fq_w_bits(out):
    d = {"bits": np.array(BITS), "n_cases": np.array(len(SHAPES))}
    for n in BITS:
        for ci, (shape, axis) in enumerate(SHAPES):
            for draw in range(64):
                case = _fq_w_case(n, ci, shape, axis, draw)
                if case is not None:
                    break
                print(f"fq_w_bits: n={n} case {ci} draw {draw}: w/delta within {TIE_MARGIN} of a half-integer, re-drawing")
            assert case is not None
            for k, v in case.items():
                d[f"n{n}.{k}{ci}"] = v
    np.savez_compressed(os.path.join(out, "fq_w_bits.npz"), **d)
    print("fq_w_bits: keys", len(d))


def gen_tiny_step_w4(out, n_steps=53, weight_n_bits=4):
    d = {}
    torch.manual_seed(0)
    kw = dict(n_spks=2, kernel_size=16, stride=8, n_filters=32, bn_chan=16, hid_chan=32, n_blocks=2, n_repeats=1)
    model = MG.ConvTasNetQ(**kw)
    fmodel = copy.deepcopy(model)
    model = MG.quantize_model(model, dict(MG.QCFG, weight_n_bits=weight_n_bits))
    model.train(); fmodel.eval()
    for m in model.modules():
        if isinstance(m, RQ.GradientWeightFakeQuantize):
            assert m.n_bits == weight_n_bits
        if isinstance(m, RQ.GradientActivationFakeQuantize):
            assert m.n_bits == 8
    for k, v in model.state_dict().items():
        d[f"sd0.{k}"] = npy(v)
    for k, v in fmodel.state_dict().items():
        d[f"fsd.{k}"] = npy(v)
    d["sd_keys"] = np.array(list(model.state_dict().keys()))
    d["weight_n_bits"] = np.array(weight_n_bits)
    x, tgt = MG.synth_batch(2, 800, seed=0)
    d["x"], d["tgt"] = npy(x), npy(tgt)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    record = {1, 2, 50, 51, 52, 53}
    d["layer_names"] = np.array([n for n, m in model.named_modules() if isinstance(m, RL.LayerQ)])
    for step in range(1, n_steps + 1):
        acts, hooks = {}, []
        if step == 51:
            # the same forward in float64 from the same (step-50) state, on copies: what the fp32 rounding of the reference itself is worth
            m64, f64 = copy.deepcopy(model).double(), copy.deepcopy(fmodel).double()
            with torch.no_grad():
                d["s51.loss_f64"] = npy(MG.common_step(m64, f64, x.double(), tgt.double())[5])
            del m64, f64
            for n, m in model.named_modules():
                if isinstance(m, RL.LayerQ):
                    hooks.append(m.register_forward_hook(
                        lambda mod, i, o, n=n: acts.__setitem__(n, (tuple(npy(t) for t in i if torch.is_tensor(t)), npy(o)))))
        opt.zero_grad()
        est, fest, w, kd, task, loss, sdrs, sdrqs = MG.common_step(model, fmodel, x, tgt)
        loss.backward()
        gnorm = torch.nn.utils.clip_grad_norm_(model.parameters(), 5.0)
        for h in hooks:
            h.remove()
        if step in record:
            p = f"s{step}."
            d[p + "est"], d[p + "fest"], d[p + "w"] = npy(est), npy(fest), npy(w)
            d[p + "kd"], d[p + "task"], d[p + "loss"], d[p + "gnorm"] = npy(kd), npy(task), npy(loss), npy(gnorm)
            if step <= 2:       # the per-parameter gradient gates cover the observer-phase steps only
                for k, prm in model.named_parameters():
                    if prm.grad is not None:
                        d[p + "grad." + k] = npy(prm.grad)
            for n, (ins, o) in acts.items():
                d[p + "act." + n] = o
                for j, t in enumerate(ins):
                    d[p + f"actin{j}." + n] = t
        opt.step()
        if step in record:
            for k, v in model.state_dict().items():
                if k.endswith("min_range") or k.endswith("max_range") or step == 50:      # full state: where step 51 starts
                    d[f"s{step}.post_sd.{k}"] = npy(v)
    np.savez_compressed(os.path.join(out, "tiny_step_w4.npz"), **d)
    print("tiny_step_w4: losses", {s: float(d[f"s{s}.loss"]) for s in sorted(record)}, "s51.loss_f64", float(d["s51.loss_f64"]),
          "keys", len(d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    a = ap.parse_args()
    gen_fq_w_bits(a.out)
    gen_tiny_step_w4(a.out)
    for f in ("fq_w_bits.npz", "tiny_step_w4.npz"):
        print(f, os.path.getsize(os.path.join(a.out, f)), "bytes")


if __name__ == "__main__":
    main()
