"""BSS-eval SDR / SIR / SAR (fqss_bss_eval) without a GPU: `kernels.bss_eval` on the CPU backend
(fqss_amd/csrc/cpu/libfqss_cpu.so, `_lib.set_backend("cpu")`) against the fp64 checker of tests/helpers_bss.py on the small shapes of
tests/test_gpu_bss_eval.py, under the same gate max(1e-6 dB, 1000 U); the inputs keep SIR and SAR between 5 and 40 dB and the
checker's spread U far below the floor (measured: U <= 1.2e-12 dB, CPU backend within 1.4e-12 dB of the checker).
`val.py` refuses to run without a device, so its line with and without `bss_eval: true` is tested in tests/test_gpu_bss_eval.py."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import helpers_bss as H


@pytest.fixture()
def cpu_backend():
    from fqss_amd import _lib
    if not os.path.exists(_lib.CPU_SO_PATH):
        subprocess.check_call(["make", "-C", os.path.dirname(_lib.CPU_SO_PATH)])
    _lib.set_backend("cpu")
    yield
    _lib.set_backend("hip")


@pytest.mark.parametrize("S,T,L", H.SHAPES)
def test_cpu_backend_bss_eval_meets_the_gate(S, T, L, cpu_backend):
    from fqss_amd import kernels as K
    est, ref = H.make_case(S, L, seed=100 * S + T)
    want, U = H.bss_ref_with_spread(est, ref, filter_length=T)
    assert U.max() <= H.FLOOR_DB / 10, "the checker is an order finer than the floor of the gate"
    if S > 1:
        assert 5.0 <= want[1:].min() and want[1:].max() <= 40.0, want
    e, r = torch.from_numpy(est), torch.from_numpy(ref)
    got = K.bss_eval(e, r, filter_length=T)
    assert got.dtype == torch.float64 and got.shape == (3, S)
    H.check(got.numpy(), want, U, f"S = {S}, T = {T}, L = {L}")
    H.check(got[0].numpy(), K.sdr(e, r, filter_length=T).numpy(), U[0], "SDR row against kernels.sdr")


def test_cpu_backend_options_pitched_rows_silent_target_and_refusals(cpu_backend):
    from fqss_amd import _lib
    from fqss_amd import kernels as K
    est, ref = H.make_case(2, 1000, seed=216)
    e, r = torch.from_numpy(est), torch.from_numpy(ref)
    want, U = H.bss_ref_with_spread(est + np.float32(0.05), ref, filter_length=16, tgt=[1, 0], zero_mean=True, load_diag=1e-3)
    H.check(K.bss_eval(e + 0.05, r, tgt=[1, 0], filter_length=16, zero_mean=True, load_diag=1e-3).numpy(), want, U, "tgt, zero_mean, load_diag")
    padded = torch.full((2, 1040), 5.0)
    padded[:, :1000] = e
    assert torch.equal(K.bss_eval(padded[:, :1000], r, filter_length=16), K.bss_eval(e, r, filter_length=16))
    silent = r.clone()
    silent[0] = 0.0
    assert torch.isnan(K.bss_eval(e, silent, filter_length=16)).all()
    for bad in (dict(est=e.repeat(2, 1), ref=r.repeat(2, 1)), dict(est=e, ref=r, filter_length=513)):
        with pytest.raises(_lib.FqssError, match="fqss_bss_eval"):
            K.bss_eval(**bad)
    assert _lib.query("fqss_bss_eval_ws_doubles", 4, 1000, 16) == 0 and _lib.query("fqss_bss_eval_ws_doubles", 2, 1000, 16) > 0
