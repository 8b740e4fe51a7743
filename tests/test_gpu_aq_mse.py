"""The histogram-MSE activation observer (`act_observer: mse`) on the HIP path: csrc/aq_mse.hip k_aq_hist / k_aq_prep / k_aq_merge /
k_aq_search / k_aq_argmin against the fp64 NumPy checker of tests/helpers_aq_mse.py (the cases tests/test_aq_mse_cpu.py runs on the CPU
backend), the reference's own ranges (tests/golden/act_mse.npz), then the module inside the tiny ConvTasNetQ of tiny_step.npz: the
observer phase against its minmax twin, 60 training steps through the hipGraph capture, two deterministic runs.

Measured on MI355X: the fixture's ranges differ from the reference's by 0 and 0 of the span; vals equal the checker's to the last bit in
all five merge cases."""
import numpy as np
import pytest
import torch

import oracle.fqss_oracle as O
from tests import helpers_aq_mse as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    yield


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("case", H.hist_inputs(), ids=lambda c: c[0])
def test_hist_counts_equal_the_checker(case):
    """n = 1 (lo == hi), 513, 4099 and 4099 one element off 16-B alignment (vector head / tail), 2^16 half zeros (wave aggregation), 2^20
    (128 workgroups, global flush), values on the checker's own edges and hi itself; rng bit for bit; obs_ws reset"""
    from fqss_amd import kernels as K
    H.check_hist_case(K, *case, "cuda")


def test_hist_two_streams_give_identical_rows():
    from fqss_amd import kernels as K
    name, x, _ = H.hist_inputs()[5]
    rows = []
    for _ in range(2):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            rows.append(H.device_hist(K, x, "cuda")[0])
        torch.cuda.current_stream().wait_stream(s)
    assert np.array_equal(rows[0], rows[1]) and np.array_equal(rows[0], H.hist(x)[0])


@pytest.mark.parametrize("case", H.VIEW_CASES, ids=lambda c: c[0])
def test_hist_reads_padded_rows_in_place(case):
    from fqss_amd import kernels as K
    H.check_hist_view_case(K, *case, "cuda")


def test_hist_void_row_and_bad_args():
    from fqss_amd import _lib, kernels as K
    x = torch.randn(1000, device="cuda")
    h, r = torch.zeros(H.BINS, dtype=torch.int32, device="cuda"), torch.zeros(2, device="cuda")
    obs = torch.tensor([-1, 0], dtype=torch.int32, device="cuda")          # nothing observed: not finite
    K.aq_hist(x, obs, h, r)
    assert int(h.sum()) == 0 and bool(torch.isnan(r).all()) and obs.tolist() == [-1, 0]
    with pytest.raises(_lib.FqssError, match="n_bits must be 8"):
        K.aq_mse_search(h.reshape(1, -1), torch.zeros(1, 2, device="cuda"), torch.zeros(1, device="cuda"), torch.ones(1, device="cuda"), n_bits=4)
    qmin, qmax = torch.tensor([-0.5], device="cuda"), torch.tensor([0.5], device="cuda")       # every row void: the ranges stay
    res = K.aq_mse_search(h.reshape(1, -1), r.reshape(1, 2), qmin, qmax, want=True)
    assert (float(qmin), float(qmax)) == (-0.5, 0.5) and res.ij.tolist() == [-1, -1] and bool(torch.isnan(res.best))


@pytest.mark.parametrize("case", H.merge_inputs(), ids=lambda c: c[0])
def test_merge_vs_checker(case):
    """T = 1, T = 50 with growing ranges, two disjoint spans, a void row among valid ones, 1e-3 beside 100 (the cap path, M = 65536)"""
    from fqss_amd import kernels as K
    H.check_merge_case(K, *case, "cuda")


@pytest.mark.parametrize("case", H.search_inputs(), ids=lambda c: c[0])
def test_search_vs_checker(case):
    from fqss_amd import kernels as K
    H.check_search_case(K, *case, "cuda")


def test_search_repeats_its_bits():
    from fqss_amd import kernels as K
    hists, rngs = H.rows_for(H.search_inputs()[0][1])
    a, b = (H.device_search(K, hists, rngs, "cuda")[0] for _ in range(2))
    assert torch.equal(a.err.view(torch.int64), b.err.view(torch.int64)) and torch.equal(a.vals.view(torch.int64), b.vals.view(torch.int64))


# ------------------------------------------------------------------------------------------------ the module
def test_reference_fixture():
    from fqss_amd import kernels as K
    H.check_reference_fixture(K, "cuda")


def test_tiny_convtasnet_observer_phase():
    """50 training forwards, minmax and mse from one seed: bit-equal outputs, the recorded (min, max) replay the EMA twin's ranges, every
    row counts its tensor, the checker's search on the device histograms gives the module's ranges"""
    from fqss_amd import kernels as K
    x, _ = O.synth_batch(2, 800, seed=5)
    H.check_model_observer_phase(K, "cuda", x)


def test_kd_step_captures_after_the_search_and_stays_finite():
    """60 steps with mse: the graphs are recorded in front of the same step as with minmax (the 52nd: 50 observing steps, one eager
    quantizing step), the searched ranges are in place by then, every loss finite"""
    la, ca, _, _ = H.kd_run(None)
    lb, cb, _, model = H.kd_run("mse")
    assert ca == cb == 51, (ca, cb)
    assert np.isfinite(lb).all() and np.isfinite(la).all()
    np.testing.assert_allclose(la[0], lb[0], rtol=1e-6)         # the observer phase does not read the ranges (later steps differ by
    #                                                             the order of the fp32 gradient atomics, run to run)
    for n, m in H.act_quantizers(model):
        if m.n_iter:
            assert not m.observing() and m._hist is None and float(m.min_range.detach()) < float(m.max_range.detach()), n


def test_deterministic_runs_end_bit_identical(monkeypatch):
    monkeypatch.setenv("FQSS_DETERMINISTIC", "1")
    (la, ca, pa, _), (lb, cb, pb, _) = H.kd_run("mse"), H.kd_run("mse")
    assert ca == cb == 51
    assert np.array_equal(la, lb) and torch.equal(pa, pb)
