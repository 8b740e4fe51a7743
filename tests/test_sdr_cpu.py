"""Signal-to-distortion ratio (fqss_sdr) without a GPU: the fp64 checker of tests/helpers_sdr.py against itself by three routes, and
`kernels.sdr` / `process.sdr` on the CPU backend (fqss_amd/csrc/cpu/libfqss_cpu.so, `_lib.set_backend("cpu")`) against the checker.

Tolerances.  The checker's routes (correlations by FFT or by direct lag sums; dense LU or scipy's Levinson solver) are the same
quantity in fp64; what they differ by is the checker's own noise.  On the grid below (AR(1) coefficient {0, 0.9, 0.99} x SNR {0, 20, 60}
dB x L {700, 2048, 6000}; condition numbers of the 512 x 512 Toeplitz matrix up to 3.1e5) the largest difference between two routes
was measured at 5.4e-9 dB.  The gate of the library, helpers_sdr.GATE_DB = 1e-6 dB, tests the library and not the checker only while
the checker is at least an order of magnitude finer than it: the routes must agree to GATE_DB / 10.  1e-6 dB covers a differently
ordered fp64 summation of up to 6000 terms amplified by 1 / (1 - coh) = 1e6 at 60 dB, and stays four orders below the two decimals
`val.py` prints.  Measured on the CPU backend: at most 4.3e-8 dB from the checker over the grid."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import helpers_sdr as H


@pytest.fixture()
def cpu_backend():
    from fqss_amd import _lib
    if not os.path.exists(_lib.CPU_SO_PATH):
        subprocess.check_call(["make", "-C", os.path.dirname(_lib.CPU_SO_PATH)])
    _lib.set_backend("cpu")
    yield
    _lib.set_backend("hip")


@pytest.fixture(scope="module")
def grid():
    """(estimate, target, checker's SDR) per case, computed once"""
    out = []
    for coef, snr, L in H.GRID:
        e, t = H.grid_case(coef, snr, L)
        out.append((coef, snr, L, e, t, H.sdr_ref(e, t)))
    return out


def test_checker_routes_agree(grid):
    worst, worst_cond = 0.0, 0.0
    for coef, snr, L, e, t, db in grid:
        alt = [H.sdr_ref(e, t, corr="direct", solver="lu"), H.sdr_ref(e, t, corr="fft", solver="levinson")]
        _, cond = H.sdr_ref(e, t, want_cond=True)
        spread = max(abs(a - db) for a in alt)
        worst, worst_cond = max(worst, spread), max(worst_cond, cond)
        assert np.isfinite(db) and spread <= H.GATE_DB / 10, (coef, snr, L, db, alt)
    print(f"checker routes: max spread {worst:.3g} dB, max cond {worst_cond:.3g}")


def test_cpu_backend_sdr_meets_the_gate_on_the_grid(grid, cpu_backend):
    from fqss_amd import kernels as K
    worst = 0.0
    for coef, snr, L, e, t, db in grid:
        got = K.sdr(torch.from_numpy(e)[None], torch.from_numpy(t)[None])
        assert got.dtype == torch.float64 and got.shape == (1,)
        err = abs(float(got[0]) - db)
        worst = max(worst, err)
        assert err <= H.GATE_DB, (coef, snr, L, float(got[0]), db)
    print(f"cpu backend vs checker: max |diff| {worst:.3g} dB")


def test_cpu_backend_sdr_options_pitched_rows_and_silent_target(cpu_backend):
    from fqss_amd import process
    from fqss_amd import kernels as K
    L = 700
    pairs = [H.grid_case(c, 20.0, L) for c in H.AR_COEFS]
    buf_e, buf_t = torch.full((3, L + 13), float("nan")), torch.full((3, L + 13), float("nan"))
    for i, (e, t) in enumerate(pairs):
        buf_e[i, 5:5 + L] = torch.from_numpy(e) + 0.05
        buf_t[i, 5:5 + L] = torch.from_numpy(t) + 0.05
    est, ref = buf_e[:, 5:5 + L], buf_t[:, 5:5 + L]
    for F in (1, 2, 64, 511, 512):
        for kw in (dict(), dict(zero_mean=True), dict(load_diag=1e-3), dict(zero_mean=True, load_diag=1e-3)):
            got = K.sdr(est, ref, filter_length=F, **kw).numpy()
            want = H.sdr_ref_rows(est.numpy(), ref.numpy(), filter_length=F, **kw)
            assert np.abs(got - want).max() <= H.GATE_DB, (F, kw, got, want)
    # L shorter than the filter
    got = K.sdr(est[:, :300], ref[:, :300]).numpy()
    assert np.abs(got - H.sdr_ref_rows(est[:, :300].numpy(), ref[:, :300].numpy())).max() <= H.GATE_DB
    # the closed form at filter_length = 1
    got = K.sdr(est, ref, filter_length=1).numpy()
    assert np.abs(got - [H.closed_form_f1(e, r) for e, r in zip(est.numpy(), ref.numpy())]).max() <= H.GATE_DB
    # process.sdr flattens leading dimensions; a silent target is NaN in its own pair only
    ref3 = ref.clone()
    ref3[1] = 0.0
    got = process.sdr(est.reshape(3, 1, L), ref3.reshape(3, 1, L)).numpy()
    want = H.sdr_ref_rows(est.numpy(), ref.numpy())
    assert got.shape == (3,) and np.isnan(got[1]) and np.abs(got[[0, 2]] - want[[0, 2]]).max() <= H.GATE_DB


def test_cpu_backend_sdr_refuses_bad_arguments(cpu_backend):
    from fqss_amd import _lib
    from fqss_amd import kernels as K
    e, t = torch.randn(2, 64), torch.randn(2, 64)
    for F in (0, 513, -1):
        with pytest.raises(_lib.FqssError, match="fqss_sdr"):
            K.sdr(e, t, filter_length=F)
    ws, db = torch.empty(4096, dtype=torch.float64), torch.full((2,), 7.0, dtype=torch.float64)
    need = _lib.query("fqss_sdr_ws_doubles", 2, 64, 8)
    assert need == 2 * 1 * (2 * 8 + 4) and _lib.query("fqss_sdr_ws_doubles", 2, 2049, 512) == 2 * 3 * 1028
    for args in ((e.data_ptr(), t.data_ptr(), ws.data_ptr(), need - 1, db.data_ptr(), 2, 64, 64, 64, 8, 0, -1.0, None),      # short workspace
                 (e.data_ptr(), t.data_ptr(), ws.data_ptr(), need, db.data_ptr(), 2, 64, 63, 64, 8, 0, -1.0, None),          # ld < L
                 (e.data_ptr(), t.data_ptr(), ws.data_ptr(), need, db.data_ptr(), 2, 0, 64, 64, 8, 0, -1.0, None),           # L < 1
                 (e.data_ptr(), None, ws.data_ptr(), need, db.data_ptr(), 2, 64, 64, 64, 8, 0, -1.0, None)):                 # null pointer
        with pytest.raises(_lib.FqssError, match="fqss_sdr"):
            _lib.call("fqss_sdr", *args)
    assert bool((db == 7.0).all())
