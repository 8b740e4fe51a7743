"""Weight quantizers at 2 to 8 bits (`weight_n_bits`) on the CPU backend (fqss_amd/csrc/cpu/libfqss_cpu.so): the width-taking entry
points fqss_wq_fwd_bits / fqss_wq_bwd_bits against the reference's own numbers (tests/golden/fq_w_bits.npz, tiny_step_w4.npz, written
by tools/make_goldens_wbits.py), the width checks of the quantizer constructors, and a W4A8 model from quantize_model down to 53
training steps.  The same bodies run on the HIP kernels in tests/test_gpu_weight_bits.py."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import helpers_wbits as H


@pytest.fixture()
def cpu_backend(monkeypatch):
    from fqss_amd import _lib, smoke
    if not os.path.exists(_lib.CPU_SO_PATH):
        subprocess.check_call(["make", "-C", os.path.dirname(_lib.CPU_SO_PATH)])
    _lib.set_backend("cpu")
    # the GPU test bodies say `.cuda()`: on this backend tensors stay on the host
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    monkeypatch.setattr(torch.nn.Module, "cuda", lambda self, *a, **k: self)
    real = smoke.build_pair
    monkeypatch.setattr(smoke, "build_pair", lambda device="cpu", seed=0, **kw: real("cpu", seed, **kw))
    yield
    _lib.set_backend("hip")


def test_fq_w_bits_goldens_bit_exact_on_the_cpu_backend(golden, cpu_backend):
    """the reference's GradientWeightFakeQuantize at n = 2 .. 7, four shape / axis cases each: codes inside [-2^(n-1), 2^(n-1) - 1],
    idx, y and gw bit for bit, gmin / gmax at the gate of test_golden_fq_w (rtol 1e-4, atol 1e-6)"""
    H.check_fq_w_bits(golden("fq_w_bits"), "cpu")


def test_width_8_reproduces_the_8_bit_goldens(golden, cpu_backend):
    """the width-taking entry points at n = 8 give fq_w.npz bit for bit: the old entry points are wrappers that pass 8, and they
    still answer the same"""
    from fqss_amd import _lib, kernels as K
    g = golden("fq_w")
    for i in range(int(g["n_cases"])):
        H.check_fq_w_case(g, "", 8, i, "cpu")
        # ... and the C entry points without a width, as a third-party binder calls them
        axis = int(g[f"axis{i}"])
        w, gr, lo, hi = (H.T(g[f"{k}{i}"]) for k in ("w", "g", "min", "max"))
        o, c, n = K._w_layout(w.shape, axis)
        y, idx = torch.empty_like(w), torch.empty(w.shape, dtype=torch.int8)
        _lib.call("fqss_wq_fwd", w.data_ptr(), y.data_ptr(), idx.data_ptr(), o, c, n, lo.data_ptr(), hi.data_ptr(), None)
        assert np.array_equal(y.numpy(), g[f"y{i}"]) and np.array_equal(idx.numpy(), g[f"idx{i}"])
        gw, gmin, gmax = torch.empty_like(w), torch.empty_like(lo), torch.empty_like(hi)
        _lib.call("fqss_wq_bwd", w.data_ptr(), gr.data_ptr(), gw.data_ptr(), gmin.data_ptr(), gmax.data_ptr(), o, c, n, lo.data_ptr(),
                  hi.data_ptr(), 0, None)
        assert np.array_equal(gw.numpy(), g[f"gw{i}"])
        assert torch.equal(gmin, K.wq_bwd(w, gr, axis, lo, hi)[1]) and torch.equal(gmax, K.wq_bwd(w, gr, axis, lo, hi, n_bits=8)[2])


def test_unsupported_widths_raise(cpu_backend):
    """weights: 2 to 8; 1 (degenerate grid) and 9 (no int8 image) raise with the supported range in the message, in the module, the
    factory, the functional form and at the C ABI.  Activations stay 8-bit."""
    from fqss_amd import _lib, kernels as K
    from fqss_amd.quantization.qat import qat_quant as QQ
    w, lo, hi = torch.randn(4, 3, 2), -torch.ones(4, 1, 1), torch.ones(4, 1, 1)
    for n in (1, 9, 0, 16, 4.5):
        with pytest.raises(NotImplementedError, match="2 to 8"):
            QQ.GradientWeightFakeQuantize(True, (4, 3, 2), n_bits=n)
        with pytest.raises(NotImplementedError, match="2 to 8"):
            QQ.get_weight_quantizer(True, (4, 3, 2), n_bits=n)
        with pytest.raises(NotImplementedError, match="2 to 8"):
            QQ.linear_quantize(w, lo, hi, n, sym=True)
    for n in (1, 9):
        with pytest.raises(_lib.FqssError, match="2..8"):
            K.wq_fwd(w, 0, lo, hi, n_bits=n)
        with pytest.raises(_lib.FqssError, match="2..8"):
            K.wq_bwd(w, w, 0, lo, hi, n_bits=n)
    for n in range(2, 9):
        assert QQ.GradientWeightFakeQuantize(True, (4, 3, 2), n_bits=n).n_bits == n
    # activations: 8 only, as before
    for n in (4, 2, 7, 16):
        with pytest.raises(NotImplementedError, match="8 only"):
            QQ.GradientActivationFakeQuantize(True, n_bits=n)
        with pytest.raises(NotImplementedError):
            QQ.get_activation_quantizer(True, n_bits=n)
        with pytest.raises(NotImplementedError):
            QQ.linear_quantize(w, torch.tensor([-1.0]), torch.tensor([1.0]), n)
    assert QQ.GradientActivationFakeQuantize(True, n_bits=8).n_bits == 8
    # the other unsupported forms keep raising whatever the width
    with pytest.raises(NotImplementedError):
        QQ.GradientWeightFakeQuantize(True, (4, 3, 2), n_bits=4, sym=False)
    with pytest.raises(NotImplementedError):
        QQ.GradientWeightFakeQuantize(True, (4, 3, 2), n_bits=4, scale_grad=True)


def test_descriptor_table_check_refuses_bad_widths():
    """the weight descriptor has 18 words, word 17 the width; the launches cannot read the device table, so runtime.QuantTables hands
    its host rows to fqss_wq_table_check before the upload: host code of the HIP library, callable without a device"""
    from fqss_amd import _lib, kernels as K
    from fqss_amd.quantization.qat import qat_quant as QQ
    assert _lib.BACKEND == "hip" and K.WQ_DESC_WORDS == 18 and QQ.WEIGHT_BITS == tuple(range(2, 9))
    assert _lib.CONSTANTS["FQSS_WQ_DESC_WORDS"] == 18 and _lib.CONSTANTS["FQSS_VERSION"] == 100      # the #defines of include/fqss.h
    row = [0] * 12 + [1, 4, 3, 0, 4]           # words 12-16: outer, C, inner, first block, ldT
    for n in range(2, 9):
        K.wq_table_check([row + [8], row + [n]])
    K.wq_table_check([])
    for n in (1, 9, 0, -4, 255):
        with pytest.raises(_lib.FqssError, match="word 17"):
            K.wq_table_check([row + [8], row + [n]])


def test_quantize_model_w4a8_structure(golden, cpu_backend):
    """quantize_model(tiny ConvTasNetQ, weight_n_bits = 4): the reference's key set, every weight quantizer at 4 bits, every activation
    quantizer at 8"""
    from fqss_amd.quantization.qat import qat_quant as QQ
    g = golden("tiny_step_w4")
    model, _ = H.tiny_pair_w4(g, "cpu")
    assert list(model.state_dict().keys()) == [str(k) for k in g["sd_keys"]]
    wq = [m for m in model.modules() if isinstance(m, QQ.GradientWeightFakeQuantize)]
    aq = [m for m in model.modules() if isinstance(m, QQ.GradientActivationFakeQuantize)]
    assert len(wq) >= 10 and all(m.n_bits == 4 for m in wq)
    assert len(aq) >= 10 and all(m.n_bits == 8 for m in aq)
    st = QQ.export_integer_state(model)
    assert all((e["quant_min"], e["quant_max"]) == (-8, 7) for k, e in st.items() if "scales" in e)
    assert all((e["quant_min"], e["quant_max"]) == (0, 255) for k, e in st.items() if "scale" in e)


def test_tiny_w4a8_training_on_the_cpu_backend(golden, cpu_backend, capsys):
    """53 W4A8 steps of the tiny pair against the reference's run: G2 gates at steps 1-2, the midpoint gate at step 53"""
    with capsys.disabled():
        H.check_tiny_training_w4(golden("tiny_step_w4"), "cpu")
