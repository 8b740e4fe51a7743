"""Shared bodies of the weight-width tests (`weight_n_bits` = 2 to 8): tests/test_weight_bits_cpu.py runs them on the CPU backend,
tests/test_gpu_weight_bits.py on the HIP kernels.  Fixtures: tests/golden/fq_w_bits.npz and tiny_step_w4.npz, both written from the
reference by tools/make_goldens_wbits.py."""
import copy

import numpy as np
import torch

import oracle.fqss_oracle as O

TINY = dict(n_spks=2, kernel_size=16, stride=8, n_filters=32, bn_chan=16, hid_chan=32, n_blocks=2, n_repeats=1)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def qcfg(weight_n_bits=4, **over):
    from fqss_amd.smoke import QCFG
    return dict(QCFG, weight_n_bits=weight_n_bits, **over)


def build_pair(device, cfg, seed=0, **kw):
    """smoke.build_pair with the quantization config of the caller"""
    from fqss_amd.quantization.qat.models.convtasnetq import ConvTasNetQ
    from fqss_amd.quantization.qat.models.load_model import quantize_model
    torch.manual_seed(seed)
    model = ConvTasNetQ(**kw)
    fmodel = copy.deepcopy(model)
    model = quantize_model(model, dict(cfg))
    return model.to(device).train(), fmodel.to(device).eval()


def tiny_pair_w4(g, device, prefix="sd0."):
    model, fmodel = build_pair(device, qcfg(int(g["weight_n_bits"])), **TINY)
    model.load_state_dict({k[len(prefix):]: T(g[k]) for k in g.files if k.startswith(prefix)}, strict=True)
    fmodel.load_state_dict({k[4:]: T(g[k]) for k in g.files if k.startswith("fsd.")}, strict=True)
    return model, fmodel


def leave_observer(model):
    from fqss_amd.quantization.qat import qat_quant as QQ
    for m in model.modules():
        if isinstance(m, QQ.GradientActivationFakeQuantize):
            m.n_iter = m.max_observations
        if isinstance(m, QQ.GradientWeightFakeQuantize):
            m.observer_mode = False


def check_fq_w_case(g, pre, n, i, device):
    """one recorded case of the reference's weight quantizer at width n: idx / y / gw bit for bit, range gradients to summation order"""
    from fqss_amd import kernels as K
    axis = int(g[f"{pre}axis{i}"])
    w, gr = T(g[f"{pre}w{i}"]).to(device), T(g[f"{pre}g{i}"]).to(device)
    lo, hi = T(g[f"{pre}min{i}"]).to(device), T(g[f"{pre}max{i}"]).to(device)
    y, idx = K.wq_fwd(w, axis, lo, hi, want_idx=True, n_bits=n)
    idx = idx.cpu().numpy()
    assert idx.dtype == np.int8 and idx.min() >= -2 ** (n - 1) and idx.max() <= 2 ** (n - 1) - 1, (n, i, idx.min(), idx.max())
    assert np.array_equal(idx, g[f"{pre}idx{i}"]), (n, i)
    assert np.array_equal(y.cpu().numpy(), g[f"{pre}y{i}"]), (n, i)
    gw, gmin, gmax = K.wq_bwd(w, gr, axis, lo, hi, n_bits=n)
    assert np.array_equal(gw.cpu().numpy(), g[f"{pre}gw{i}"]), (n, i)
    np.testing.assert_allclose(gmin.cpu().numpy(), g[f"{pre}gmin{i}"], rtol=1e-4, atol=1e-6, err_msg=f"n={n} case {i}")
    np.testing.assert_allclose(gmax.cpu().numpy(), g[f"{pre}gmax{i}"], rtol=1e-4, atol=1e-6, err_msg=f"n={n} case {i}")
    # the accumulating form the autograd node uses: += onto given buffers
    acc = (torch.ones_like(w), torch.ones_like(lo), torch.ones_like(hi))
    K.wq_bwd(w, gr, axis, lo, hi, out=acc, n_bits=n)
    assert torch.equal(acc[0], gw + 1.0)
    # the functional form of the reference (linear_quantize, sym=True) through autograd
    from fqss_amd.quantization.qat import qat_quant as QQ
    wr, lr, hr = w.clone().requires_grad_(True), lo.clone().requires_grad_(True), hi.clone().requires_grad_(True)
    yf = QQ.linear_quantize(wr, lr, hr, n, sym=True)
    yf.backward(gr)
    assert torch.equal(yf.detach(), y) and torch.equal(wr.grad, gw)
    assert torch.equal(lr.grad, gmin) and torch.equal(hr.grad, gmax)


def check_fq_w_bits(g, device):
    bits = [int(n) for n in g["bits"]]
    assert bits == [2, 3, 4, 5, 6, 7]
    for n in bits:
        for i in range(int(g["n_cases"])):
            check_fq_w_case(g, f"n{n}.", n, i, device)


def check_tiny_training_w4(g, device):
    """KDTrainStep on the tiny W4A8 pair against the reference's 53 steps (tiny_step_w4.npz): the G2 gates of
    test_gpu_model.test_tiny_training_vs_reference_goldens at steps 1-2; at step 53 the loss must be below the midpoint between
    the reference's step-1 and step-53 losses -- it trains as the reference did.  (The 3.5 dB late-step gate of the 8-bit test is a
    measured cross-machine spread of 8-bit grids; nobody has measured it at 4 bits, so it is not reused.)"""
    from fqss_amd.quantization.qat import qat_quant as QQ
    from fqss_amd.runtime import KDTrainStep
    model, fmodel = tiny_pair_w4(g, device)
    assert all(m.n_bits == 4 for m in model.modules() if isinstance(m, QQ.GradientWeightFakeQuantize))
    step = KDTrainStep(model, fmodel, kd_lambda=0.1, lr=1e-3, clip=5.0)
    x, tgt = T(g["x"]).to(device), T(g["tgt"]).to(device)
    for s in range(1, 54):
        r = step(x, tgt)
        p = f"s{s}."
        if s > 2:
            continue
        est = r["est"].cpu().numpy()
        print(f"step {s}: loss {r['loss'].item():.6f} (reference {float(g[p + 'loss']):.6f}), kd {r['kd'].item():.6f} "
              f"({float(g[p + 'kd']):.6f}), gnorm {r['gnorm'].item():.6f} ({float(g[p + 'gnorm']):.6f})")
        np.testing.assert_allclose(r["loss"].item(), g[p + "loss"], rtol=1e-5, err_msg=p)
        np.testing.assert_allclose(r["kd"].item(), g[p + "kd"], rtol=1e-5, err_msg=p)
        np.testing.assert_allclose(r["w"].cpu().numpy(), g[p + "w"], rtol=2.3e-4, err_msg=p)
        np.testing.assert_allclose(est, g[p + "est"], rtol=1e-4, atol=2e-6, err_msg=p)
        np.testing.assert_allclose(r["gnorm"].item(), g[p + "gnorm"], rtol=1e-4, err_msg=p)
        coef = min(1.0, 5.0 / (float(g[p + "gnorm"]) + 1e-6))     # the fixture holds the clipped gradients
        n_checked, worst = 0, 0.0
        for name, prm in model.named_parameters():
            k = p + "grad." + name
            if k in g.files:
                ref = g[k] / coef
                err = np.linalg.norm(prm.grad.cpu().numpy() - ref) / (np.linalg.norm(ref) + 1e-12)
                worst = max(worst, err)
                assert err <= 2e-3, (k, err)
                n_checked += 1
            else:
                assert float(prm.grad.abs().max()) == 0.0, name      # reference: grad is None
        assert n_checked >= 30
        print(f"step {s}: worst normwise gradient error {worst:.3e} over {n_checked} parameters")
    first, last = float(g["s1.loss"]), float(g["s53.loss"])
    bound = 0.5 * (first + last)
    print(f"step 53: loss {r['loss'].item():.4f}; reference {first:.4f} -> {last:.4f}, midpoint {bound:.4f}")
    assert last < first and r["loss"].item() < bound, (r["loss"].item(), bound)


def mixed_widths(model, tcn_bits=4, other_bits=8):
    """set by hand: the TCN's weight quantizers at `tcn_bits`, every other one (encoder, bottleneck, mask conv, decoder) at `other_bits`"""
    from fqss_amd.quantization.qat import qat_quant as QQ
    n = {tcn_bits: 0, other_bits: 0}
    for name, m in model.named_modules():
        if isinstance(m, QQ.GradientWeightFakeQuantize):
            m.n_bits = tcn_bits if ".TCN." in name else other_bits
            n[m.n_bits] += 1
    assert n[tcn_bits] > 0 and n[other_bits] > 0, n
    return model


def si_sdr_db(est, tgt):
    return float(O.si_sdr_db(est, tgt))
