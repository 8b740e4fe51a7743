"""The MSE weight observer (`weight_observer: mse`) on the CPU backend (fqss_amd/csrc/cpu/libfqss_cpu.so): fqss_wq_observe_mse and
fqss_wq_error against the NumPy oracle of tests/helpers_wq_mse.py, then a tiny ConvTasNet from quantize_model down to training steps and
the report.  The same bodies run on the HIP kernels in tests/test_gpu_wq_mse.py."""
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle.fqss_oracle as O
from tests import helpers_wq_mse as H


@pytest.fixture()
def cpu_backend(monkeypatch):
    from fqss_amd import _lib, smoke
    if not os.path.exists(_lib.CPU_SO_PATH):
        subprocess.check_call(["make", "-C", os.path.dirname(_lib.CPU_SO_PATH)])
    _lib.set_backend("cpu")
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    monkeypatch.setattr(torch.nn.Module, "cuda", lambda self, *a, **k: self)
    real = smoke.build_pair
    monkeypatch.setattr(smoke, "build_pair", lambda device="cpu", seed=0, **kw: real("cpu", seed, **kw))
    yield
    _lib.set_backend("hip")


def _cases(kind, layout):
    return [c for c in H.cases() if c[0] == kind and c[1] == layout]


@pytest.mark.parametrize("n_bits", H.BITS)
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("kind", H.KINDS)
def test_observe_mse_vs_oracle(cpu_backend, kind, layout, n_bits):
    """chosen k, ranges bit for bit, e_0 and e_k at 1e-12, two runs bit-equal, candidate 0 == fqss_wq_observe; all-zero -> (0, 0)"""
    from fqss_amd import kernels as K
    assert _cases(kind, layout)
    for case in _cases(kind, layout):
        ks, _ = H.check_observe_case(K, *case, n_bits, "cpu")
        if kind == "uniform" and n_bits == 8:
            assert max(ks) <= 2, (case, ks)          # nothing to clip: k = 0 or next to it


@pytest.mark.parametrize("n_bits", H.BITS)
@pytest.mark.parametrize("layout", [0, 1])
def test_wq_error_vs_oracle(cpu_backend, layout, n_bits):
    from fqss_amd import kernels as K
    for kind in ("gauss", "laplace"):
        for C, n in ((1, 1), (3, 65), (300, 257), (3, 1536), (1, H.STAGE + 1)):
            H.check_error_case(K, kind, layout, C, n, n_bits, "cpu")


def test_tie_rule(cpu_backend):
    from fqss_amd import kernels as K
    H.check_tie_rule(K, "cpu")


def test_bad_widths_raise(cpu_backend):
    from fqss_amd import _lib, kernels as K
    H.check_bad_args(K, _lib.FqssError, pytest, "cpu")


def test_header_constants():
    from fqss_amd import _lib, kernels as K
    assert (_lib.CONSTANTS["FQSS_WQ_MSE_STEPS"], _lib.CONSTANTS["FQSS_WQ_MSE_DEN"]) == (H.STEPS, H.DEN) == (K.WQ_MSE_STEPS, K.WQ_MSE_DEN)
    assert {"fqss_wq_observe_mse", "fqss_wq_error"} <= set(_lib.EXPORTS)


@pytest.mark.parametrize("n_bits", [2, 4])
def test_tiny_convtasnet_mse_observer(cpu_backend, n_bits):
    """quantize_model(weight_observer: mse) -> first training forward -> oracle ranges on every weight quantizer, the min/max model's
    keys, a strictly lower weight error than min/max, then five finite training steps; the report against the oracle"""
    from fqss_amd import kernels as K
    from fqss_amd.quantization.qat.qat_utils import weight_quant_report
    ref_model, _ = H.tiny_convtasnet("cpu", n_bits, observer=None)
    model, fmodel = H.tiny_convtasnet("cpu", n_bits, observer="mse")
    x, tgt = O.synth_batch(2, 800, seed=5)
    model(x)
    tot, tot0 = H.check_ranges_after_first_forward(K, model, ref_model.state_dict().keys(), n_bits)
    print(f"W{n_bits}: summed squared weight error {tot:.6g} with the MSE observer, {tot0:.6g} with min/max")
    H.check_report(model, weight_quant_report(model))
    H.check_five_steps(model, fmodel, x, tgt, dict(kd_lambda=0.1, lr=1e-3, clip=5.0))


def test_weight_observer_config_key(cpu_backend, monkeypatch):
    """absent / minmax: today's observer and not one call of the new entry point; mse: the new one only; anything else: ValueError"""
    from fqss_amd import _lib
    x, _ = O.synth_batch(1, 800, seed=6)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    for observer, want, never in ((None, "fqss_wq_observe", "fqss_wq_observe_mse"), ("minmax", "fqss_wq_observe", "fqss_wq_observe_mse"),
                                  ("mse", "fqss_wq_observe_mse", "fqss_wq_observe")):
        model, _ = H.tiny_convtasnet("cpu", 4, observer=observer)
        wqs = H.weight_quantizers(model)
        assert wqs and all(m.observer == (observer or "minmax") for m in wqs)
        del calls[:]
        model(x)
        model(x)
        assert calls.count(want) == len(wqs) and calls.count(never) == 0, (observer, calls.count(want), calls.count(never))
    for bad in ("bogus", "MSE", "", 0):
        with pytest.raises(ValueError, match="'minmax' or 'mse'"):
            H.tiny_convtasnet("cpu", 4, observer=bad)
    from fqss_amd.quantization.qat import qat_quant as QQ
    q = QQ.GradientWeightFakeQuantize(True, (4, 3, 2), n_bits=4)
    assert q.observer == "minmax" and list(q.state_dict()) == ["min_range", "max_range"]
    q.observer = "bogus"
    with pytest.raises(ValueError, match="'minmax' and 'mse'"):
        q(torch.randn(4, 3, 2))


def test_w4_mse_config_file():
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    a = yaml.safe_load(open(os.path.join(root, "configs", "convtasnet_2spks_8k_synthetic_w4_mse.yaml")))
    b = yaml.safe_load(open(os.path.join(root, "configs", "convtasnet_2spks_8k_synthetic_w4.yaml")))
    assert a["model_cfg"]["quantization"].pop("weight_observer") == "mse" and a["work_dir"] != b["work_dir"]
    a["work_dir"] = b["work_dir"]
    assert a == b


def test_selftest_under_address_sanitizer():
    """csrc/cpu/selftest_wq_mse.cpp: the CPU library's source under -fsanitize=address,undefined, both entry points on both layouts"""
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fqss_amd", "csrc", "cpu")
    p = subprocess.run(["make", "-C", d, "asan_wq_mse"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "selftest_wq_mse ok" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
