"""The MSE weight observer (`weight_observer: mse`) on the HIP path: csrc/fq.hip k_wq_observe_mse / k_wq_error against the NumPy oracle of
tests/helpers_wq_mse.py (the cases tests/test_wq_mse_cpu.py runs on the CPU backend), then through quantize_model on the four model
families: oracle ranges after the first training forward, training steps, a hipGraph replay, the report."""
import numpy as np
import pytest
import torch

import oracle.fqss_oracle as O
from tests import helpers_wq_mse as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    yield


def _cases(kind, layout):
    return [c for c in H.cases() if c[0] == kind and c[1] == layout]


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("n_bits", H.BITS)
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("kind", H.KINDS)
def test_observe_mse_vs_oracle(kind, layout, n_bits):
    """chosen k, ranges bit for bit, e_0 and e_k at 1e-12, two runs bit-equal, candidate 0 == fqss_wq_observe; all-zero -> (0, 0).
    Lengths 1 .. 257 and 1536 are staged in LDS, 8193 is re-read from memory; 1, 3 and 300 workgroups.  (A 50 sigma outlier keeps
    k = 0 by the oracle too: clipping it costs more than the whole channel's rounding error down to r = 0.2.)"""
    from fqss_amd import kernels as K
    assert _cases(kind, layout)
    for case in _cases(kind, layout):
        ks, _ = H.check_observe_case(K, *case, n_bits, "cuda")
        if kind == "uniform" and n_bits == 8:
            assert max(ks) <= 2, (case, ks)          # nothing to clip: k = 0 or next to it


@pytest.mark.parametrize("n_bits", H.BITS)
@pytest.mark.parametrize("layout", [0, 1])
def test_wq_error_vs_oracle(layout, n_bits):
    from fqss_amd import kernels as K
    for kind in ("gauss", "laplace"):
        for C, n in ((1, 1), (3, 65), (300, 257), (3, 1536), (1, H.STAGE + 1)):
            H.check_error_case(K, kind, layout, C, n, n_bits, "cuda")


def test_tie_rule():
    from fqss_amd import kernels as K
    H.check_tie_rule(K, "cuda")


def test_bad_widths_raise():
    from fqss_amd import _lib, kernels as K
    H.check_bad_args(K, _lib.FqssError, pytest, "cuda")


# ------------------------------------------------------------------------------------------------ through the model
def _batch(name, golden):
    if name == "htdemucs":
        g = golden("hd_tiny_step")
        return H.T(g["mix"]).cuda(), H.T(g["src"]).cuda()
    x, tgt = O.synth_batch(2, 800, seed=5) if name == "convtasnet" else O.synth_batch(1, 4000, seed=3)
    return x.cuda(), tgt.cuda()


@pytest.mark.parametrize("name,n_bits", [("convtasnet", 2), ("convtasnet", 4), ("dptnet", 4), ("sepformer", 4), ("htdemucs", 4)])
def test_family_mse_observer(golden, name, n_bits, capsys):
    """quantize_model(weight_observer: mse) on a tiny build of each family -> first training forward -> the oracle's ranges on every
    weight quantizer (conv, transposed conv, conv2d, attention projections, LSTM matrices, embedding), observer_mode off, the min/max
    model's keys, per-channel error <= min/max and strictly lower in total; the report against the oracle; five finite steps"""
    from fqss_amd import kernels as K
    from fqss_amd.quantization.qat.qat_utils import weight_quant_report
    ref_keys = list(H.family_pair(name, "cpu", n_bits, observer=None)[0].state_dict().keys())
    model, fmodel, step_kw = H.family_pair(name, "cuda", n_bits, observer="mse")
    x, tgt = _batch(name, golden)
    with torch.no_grad():
        model(x)
    tot, tot0 = H.check_ranges_after_first_forward(K, model, ref_keys, n_bits)
    with capsys.disabled():
        print(f"{name} W{n_bits}: summed squared weight error {tot:.6g} with the MSE observer, {tot0:.6g} with min/max")
    H.check_report(model, weight_quant_report(model))
    H.check_five_steps(model, fmodel, x, tgt, step_kw)


def test_weight_observer_config_key(monkeypatch):
    """absent / minmax: today's observer and not one call of the new entry point; mse: the new one only; anything else: ValueError"""
    from fqss_amd import _lib
    x, _ = O.synth_batch(1, 800, seed=6)
    x = x.cuda()
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    for observer, want, never in ((None, "fqss_wq_observe", "fqss_wq_observe_mse"), ("minmax", "fqss_wq_observe", "fqss_wq_observe_mse"),
                                  ("mse", "fqss_wq_observe_mse", "fqss_wq_observe")):
        model, _ = H.tiny_convtasnet("cuda", 4, observer=observer)
        wqs = H.weight_quantizers(model)
        assert wqs and all(m.observer == (observer or "minmax") for m in wqs)
        del calls[:]
        with torch.no_grad():
            model(x)
            model(x)
        assert calls.count(want) == len(wqs) and calls.count(never) == 0, (observer, calls.count(want), calls.count(never))
    with pytest.raises(ValueError, match="'minmax' or 'mse'"):
        H.tiny_convtasnet("cuda", 4, observer="bogus")


def test_hipgraph_replay_matches_eager_w4_mse():
    """the body of test_gpu_weight_bits.test_hipgraph_replay_matches_eager_w4a8 on a pair whose weight ranges the MSE observer wrote:
    the search runs in the first forward, before any capture; the captured step replays to the eager result"""
    from fqss_amd.quantization.qat import qat_quant as QQ
    from fqss_amd.runtime import KDTrainStep
    x, tgt = _batch("convtasnet", None)
    runs = []
    for use_graph in (False, True):
        model, fmodel = H.tiny_convtasnet("cuda", 4, observer="mse")
        with torch.no_grad():
            model(x)
        assert all(not m.observer_mode for m in H.weight_quantizers(model))
        for m in model.modules():
            if isinstance(m, QQ.GradientActivationFakeQuantize):
                m.n_iter = m.max_observations
        step = KDTrainStep(model, fmodel)
        losses = [step(x, tgt)["loss"].item()]
        if use_graph:
            step.capture(x, tgt, warmup=1)
        else:
            step(x, tgt)
        for _ in range(3):
            losses.append(step(x, tgt)["loss"].item())
        runs.append((losses, step.arena.flat_p.clone()))
    (l0, p0), (l1, p1) = runs
    np.testing.assert_allclose(l0[0], l1[0], rtol=1e-6)
    np.testing.assert_allclose(l0[1:], l1[1:], atol=0.05)          # dB; chaotic after the first quantized update
    assert float((p0 - p1).abs().max()) < 5e-3
