"""The histogram-MSE activation observer (`act_observer: mse`) on the CPU backend (fqss_amd/csrc/cpu/libfqss_cpu.so): fqss_aq_hist and
fqss_aq_mse_search against the fp64 NumPy checker of tests/helpers_aq_mse.py, the reference's own ranges (tests/golden/act_mse.npz),
the module inside a tiny ConvTasNetQ, a resume from inside the observer phase, the configuration key.  The same bodies run on the HIP
kernels in tests/test_gpu_aq_mse.py.

Measured on the CPU backend: the fixture's ranges differ from the reference's by 0 and 0 of the span (the fp64 edges leave (i, j) and M
unchanged and the winner rounds to the same fp32 pair)."""
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle.fqss_oracle as O
from tests import helpers_aq_mse as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def cpu_backend():
    from fqss_amd import _lib
    if not os.path.exists(_lib.CPU_SO_PATH):
        subprocess.check_call(["make", "-C", os.path.dirname(_lib.CPU_SO_PATH)])
    prev = _lib.BACKEND
    _lib.set_backend("cpu")
    yield
    _lib.set_backend(prev)


def test_header_and_exports():
    from fqss_amd import _lib, kernels as K
    assert (K.AQ_HIST_BINS, K.AQ_MSE_MAX_ROWS, K.AQ_MSE_MAX_BINS, K.AQ_MSE_N) == (H.BINS, H.MAX_ROWS, H.MAX_M, H.N)
    assert {"fqss_aq_hist", "fqss_aq_hist_rows", "fqss_aq_mse_search", "fqss_aq_mse_ws_bytes", "fqss_aq_mse_ws_offset"} <= set(_lib.EXPORTS)
    assert _lib.query("fqss_aq_mse_ws_offset", 0, 0) == -1 and _lib.query("fqss_aq_mse_ws_offset", 3, 9) == -1


@pytest.mark.parametrize("case", H.hist_inputs(), ids=lambda c: c[0])
def test_hist_counts_equal_the_checker(cpu_backend, case):
    from fqss_amd import kernels as K
    H.check_hist_case(K, *case, "cpu")


@pytest.mark.parametrize("case", H.VIEW_CASES, ids=lambda c: c[0])
def test_hist_reads_padded_rows_in_place(cpu_backend, case):
    from fqss_amd import kernels as K
    H.check_hist_view_case(K, *case, "cpu")


def test_hist_void_row_and_bad_args(cpu_backend):
    from fqss_amd import _lib, kernels as K
    x = torch.randn(100)
    h, r = torch.zeros(H.BINS, dtype=torch.int32), torch.zeros(2)
    obs = torch.tensor([-1, 0], dtype=torch.int32)              # nothing observed: not finite
    K.aq_hist(x, obs, h, r)
    assert int(h.sum()) == 0 and bool(torch.isnan(r).all()) and obs.tolist() == [-1, 0]
    with pytest.raises(_lib.FqssError):
        K.aq_hist(x, obs, torch.zeros(100, dtype=torch.int32), r)
    with pytest.raises(_lib.FqssError):
        K.aq_hist(x.double(), obs, h, r)                        # not fp32
    with pytest.raises(_lib.FqssError, match="obs_ws"):
        K.aq_hist(x, obs.float(), h, r)
    with pytest.raises(_lib.FqssError, match="n_bits must be 8"):
        K.aq_mse_search(h.reshape(1, -1), torch.zeros(1, 2), torch.zeros(1), torch.ones(1), n_bits=4)
    with pytest.raises(_lib.FqssError):
        K.aq_mse_search(torch.zeros(65, H.BINS, dtype=torch.int32), torch.zeros(65, 2), torch.zeros(1), torch.ones(1))
    qmin, qmax = torch.tensor([-0.5]), torch.tensor([0.5])      # every row void: the ranges stay
    res = K.aq_mse_search(h.reshape(1, -1), r.reshape(1, 2), qmin, qmax, want=True)
    assert (float(qmin), float(qmax)) == (-0.5, 0.5) and res.ij.tolist() == [-1, -1] and bool(torch.isnan(res.best))


@pytest.mark.parametrize("case", H.merge_inputs(), ids=lambda c: c[0])
def test_merge_vs_checker(cpu_backend, case):
    from fqss_amd import kernels as K
    H.check_merge_case(K, *case, "cpu")


@pytest.mark.parametrize("case", H.search_inputs(), ids=lambda c: c[0])
def test_search_vs_checker(cpu_backend, case):
    from fqss_amd import kernels as K
    H.check_search_case(K, *case, "cpu")


def test_reference_fixture(cpu_backend):
    from fqss_amd import kernels as K
    H.check_reference_fixture(K, "cpu")


def test_tiny_convtasnet_observer_phase(cpu_backend):
    from fqss_amd import kernels as K
    x, _ = O.synth_batch(2, 800, seed=5)
    H.check_model_observer_phase(K, "cpu", x)


def test_resume_inside_the_observer_phase_ends_at_the_same_ranges(cpu_backend, tmp_path):
    """world 1: a checkpoint written at step 20 carries the MSE quantizers' _hist / _hist_rng rows; the resumed run's ranges after step 52
    equal the uninterrupted run's"""
    from fqss_amd import checkpoint
    from fqss_amd.runtime import KDTrainStep
    x, tgt = O.synth_batch(2, 800, seed=5)

    def fresh():
        model, fmodel = H.tiny_pair("cpu", "mse")
        return model, fmodel, KDTrainStep(model, fmodel, kd_lambda=0.1, lr=1e-3, clip=5.0)

    ma, fa, sa = fresh()
    path = str(tmp_path / "checkpoint.pth")
    for s in range(52):
        if s == 20:
            checkpoint.save_training_state(path, sa, {"epoch": 0}, fa)
        sa(x, tgt)
    ck = checkpoint.load_training_state(path)
    assert any(k.endswith("._hist") for k in ck["step"]["buffers"]) and any(k.endswith("._hist_rng") for k in ck["step"]["buffers"])
    mb, fb, sb = fresh()
    checkpoint.restore(ck, sb, fb)
    for s in range(20, 52):
        sb(x, tgt)
    qa, qb = H.act_quantizers(ma), H.act_quantizers(mb)
    assert qa and all(not m.observing() for _, m in qa if m.n_iter)
    for (n, a), (_, b) in zip(qa, qb):
        assert a.n_iter == b.n_iter and a._hist is None and (b._hist is None or b.n_iter == 0), n
        assert torch.equal(a.min_range, b.min_range) and torch.equal(a.max_range, b.max_range), n
    # a file written after the phase holds no histograms and loads into a fresh (scratch-holding) model
    checkpoint.save_training_state(path, sa, {"epoch": 0}, fa)
    ck = checkpoint.load_training_state(path)
    for n, m in qa:                                             # (a quantizer the forward never reaches keeps its empty scratch)
        assert ((n + "._hist") in ck["step"]["buffers"]) == (m.n_iter == 0), n
    mc, fc, sc = fresh()
    checkpoint.restore(ck, sc, fc)
    assert all(m._hist is None for _, m in H.act_quantizers(mc) if m.n_iter)


def test_state_dict_refuses_world_2_inside_the_observer_phase(cpu_backend):
    from fqss_amd.runtime import KDTrainStep
    model, fmodel = H.tiny_pair("cpu", "mse")
    step = KDTrainStep(model, fmodel, kd_lambda=0.1, lr=1e-3, clip=5.0)
    step._world = lambda: 2
    with pytest.raises(NotImplementedError, match="histograms"):
        step.state_dict()


def test_errors(cpu_backend):
    """act_observer: foo -> ValueError; mse on DPTNetQ / SepformerQ / HTDemucsQ -> NotImplementedError; an OBSERVE after_forward without an
    output -> RuntimeError; absent / minmax build the EMA quantizer"""
    from fqss_amd import ops
    from fqss_amd.quantization.qat import qat_quant as QQ
    from fqss_amd.quantization.qat.models.dptnetq import DPTNetQ
    from fqss_amd.quantization.qat.models.htdemucsq import HTDemucsQ
    from fqss_amd.quantization.qat.models.load_model import quantize_model
    from fqss_amd.quantization.qat.models.sepformerq import SepformerQ
    from fqss_amd.smoke import QCFG
    for bad in ("foo", "MSE", "", 0):
        with pytest.raises(ValueError, match="'minmax' or 'mse'"):
            H.tiny_pair("cpu", bad)
    for obs in (None, "minmax"):
        assert all(type(m) is QQ.GradientActivationFakeQuantize for _, m in H.act_quantizers(H.tiny_pair("cpu", obs)[0]))
    assert type(QQ.get_activation_quantizer(True)) is QQ.GradientActivationFakeQuantize          # the factory itself builds the EMA quantizer
    for build in (lambda: DPTNetQ(n_spks=2, kernel_size=2), lambda: SepformerQ(n_spks=2, kernel_size=16, stride=8),
                  lambda: HTDemucsQ(sources=["a", "b"])):
        with pytest.raises(NotImplementedError, match="ConvTasNetQ only"):
            quantize_model(build(), dict(QCFG, act_observer="mse"))
    q = H.mse_quantizer("cpu")
    assert isinstance(q, QQ.GradientActivationFakeQuantize)
    ctx = q.qctx()
    assert ctx.qmode == ops.Q_OBSERVE and ctx.out is None
    with pytest.raises(RuntimeError, match="without handing over its output"):
        q.after_forward(ctx)


def test_amse_config_file():
    import yaml
    a = yaml.safe_load(open(os.path.join(ROOT, "configs", "convtasnet_2spks_8k_synthetic_amse.yaml")))
    b = yaml.safe_load(open(os.path.join(ROOT, "configs", "convtasnet_2spks_8k_synthetic.yaml")))
    assert a["model_cfg"]["quantization"].pop("act_observer") == "mse" and a["work_dir"] != b["work_dir"]
    a["work_dir"] = b["work_dir"]
    assert a == b


def test_selftest_under_address_sanitizer():
    """csrc/cpu/selftest_aq_mse.cpp: the CPU library's source under -fsanitize=address,undefined, a stand-alone host program"""
    d = os.path.join(ROOT, "fqss_amd", "csrc", "cpu")
    p = subprocess.run(["make", "-C", d, "asan_aq_mse"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "selftest_aq_mse ok" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
