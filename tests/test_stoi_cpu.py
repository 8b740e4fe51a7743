"""Short-time objective intelligibility (fqss_stoi) without a GPU: the fp64 checker of tests/helpers_stoi.py against itself and against
what this machine has (scipy's resample_poly), and `kernels.stoi` / `process.stoi` on the CPU backend
(fqss_amd/csrc/cpu/libfqss_cpu.so, `_lib.set_backend("cpu")`) against the checker.

Tolerance.  Both sides are fp64, so the gate is an absolute difference on d.  It comes from the checker: S = the largest difference
between its two spectrum routes (numpy.fft.rfft / an explicit DFT-matrix product) over the grid, and the library must stay within
helpers_stoi.gate(S) = max(1e-12, 1000 S).  Three decades cover another FFT factorisation and other summation orders (the polyphase
branch of the resampler, segment sums); the floor of 1e-12 is still five decades below what a single fp32 intermediate would cost
(about 1e-7).  Measured here: S = 3.3e-16, CPU backend at most 5.6e-16 from the checker over the grid.

Input conditions, asserted so that no case passes by luck: the mask margin min_i |e_i - (max(e) - 40)| is at least 0.1 dB (a last-bit
difference in log10 cannot flip a frame), between 30 % and 90 % of the frames are kept, and the noisy cases land strictly between 0.5
and 0.999.  The recipe of helpers_stoi.voiced gives 50 of 69 frames, margins of 4.2 dB and more, d from 0.58 to 0.99."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import helpers_stoi as H


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
    """[(fs, snr, est, ref, d, kept frames, frames, margin, d by the DFT-matrix route)], computed once"""
    out = []
    for fs, snr in H.GRID:
        e, r = H.grid_case(fs, snr)
        d, kept, margin = H.stoi_ref(e, r, fs, want_info=True)
        p, q = H.ratio(fs)
        frames = len(H.frame_starts(-(-len(r) * p // q)))
        out.append((fs, snr, e, r, d, kept, frames, margin, H.stoi_ref(e, r, fs, dft="matrix")))
    return out


def spread(grid):
    return max(abs(c[4] - c[8]) for c in grid)


def test_checker_resampler_matches_scipy():
    signal = pytest.importorskip("scipy.signal")
    for fs, taps in ((8000, 365), (16000, 581)):
        p, q = H.ratio(fs)
        h = H.resample_window(p, q)
        assert len(h) == taps and abs(h.sum() - 1.0) < 1e-15
        for L in (H.GRID_LENGTHS[fs], H.GRID_LENGTHS[fs] - 3, 37):
            x = H.voiced(max(L, 64), fs, 4)[:L]
            mine, theirs = H.resample(x, p, q), signal.resample_poly(x.astype(np.float64), p, q, window=h)
            assert mine.shape == theirs.shape == (-(-L * p // q),)
            assert np.abs(mine - theirs).max() <= 1e-12, (fs, L)


def test_checker_routes_agree_and_the_inputs_meet_their_conditions(grid):
    for fs, snr, e, r, d, kept, frames, margin, d_matrix in grid:
        assert margin >= 0.1, (fs, snr, margin)
        assert 0.3 * frames <= kept <= 0.9 * frames, (fs, snr, kept, frames)
        assert 0.5 < d < 0.999, (fs, snr, d)
    S = spread(grid)
    print(f"checker routes: spread S = {S:.3g}, gate = {H.gate(S):.3g}")
    assert S <= 1e-13, S          # the checker is finer than the floor of the gate by a decade
    for fs in H.RATES:
        ds = [c[4] for c in grid if c[0] == fs]
        assert ds[0] > ds[1] > ds[2], (fs, ds)           # 20 / 5 / -5 dB
        r = next(c[3] for c in grid if c[0] == fs)
        assert abs(H.stoi_ref(r, r, fs) - 1.0) <= 1e-12
    lo, hi = H.band_edges()
    assert lo == [7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174] and hi == lo[1:] + [219]


def test_cpu_backend_stoi_meets_the_gate_on_the_grid(grid, cpu_backend):
    from fqss_amd import kernels as K
    gate, worst = H.gate(spread(grid)), 0.0
    for fs, snr, e, r, d, *_ in grid:
        got = K.stoi(torch.from_numpy(e)[None], torch.from_numpy(r)[None], fs)
        assert got.dtype == torch.float64 and got.shape == (1,)
        err = abs(float(got[0]) - d)
        worst = max(worst, err)
        assert err <= gate, (fs, snr, float(got[0]), d)
    print(f"cpu backend vs checker: max |diff| {worst:.3g}")


def test_cpu_backend_stoi_frame_rule_edges_pitched_rows_and_short_inputs(grid, cpu_backend):
    from fqss_amd import process
    from fqss_amd import kernels as K
    gate = H.gate(spread(grid))
    # 10 kHz without a silent stretch: 256 + 128 k samples drop the frame that ends at the last sample; 31 kept frames are one segment,
    # 30 are none
    for L, frames in ((256 + 128 * 34, 34), (256 + 128 * 34 + 1, 35), (256 + 128 * 30 + 1, 31), (256 + 128 * 30, 30)):
        ref = H.voiced(L, 10000, 77, silence=())
        est = H.noisy(ref, 5.0, 78)
        want, kept, margin = H.stoi_ref(est, ref, 10000, want_info=True)
        assert kept == frames and margin >= 0.1
        got = float(K.stoi(torch.from_numpy(est)[None], torch.from_numpy(ref)[None], 10000)[0])
        assert (got == 1e-5 and want == 1e-5) if frames == 30 else abs(got - want) <= gate, (L, got, want)
    # three pairs as the middle columns of a NaN-filled buffer, lengths that are no multiple of `down`, leading dimensions flattened
    for fs, L in ((8000, 7203), (16000, 14405)):
        cases = [H.grid_case(fs, snr, L) for snr in H.SNRS_DB]
        buf_e, buf_r = torch.full((3, L + 13), float("nan")), torch.full((3, L + 13), float("nan"))
        for i, (e, r) in enumerate(cases):
            buf_e[i, 5:5 + L] = torch.from_numpy(e)
            buf_r[i, 5:5 + L] = torch.from_numpy(r)
        want = np.array([H.stoi_ref(e, r, fs) for e, r in cases])
        got = K.stoi(buf_e[:, 5:5 + L], buf_r[:, 5:5 + L], fs).numpy()
        assert np.abs(got - want).max() <= gate, (fs, got, want)
        got = process.stoi(buf_e[:, 5:5 + L].reshape(3, 1, L), buf_r[:, 5:5 + L].reshape(3, 1, L), fs)
        assert got.shape == (3,) and np.abs(got.numpy() - want).max() <= gate
    # fewer than 30 spectral frames, no frame at all, an all-zero reference
    e, r = grid[0][2], grid[0][3]
    for fs, L in ((10000, 200), (10000, 256), (10000, 257), (8000, 200), (16000, 1)):
        assert float(K.stoi(torch.from_numpy(e[:L])[None], torch.from_numpy(r[:L])[None], fs)[0]) == 1e-5
    zero = np.zeros_like(r)
    want = H.stoi_ref(e, zero, 10000)
    assert np.isfinite(want) and abs(float(K.stoi(torch.from_numpy(e)[None], torch.from_numpy(zero)[None], 10000)[0]) - want) <= gate


def test_cpu_backend_stoi_refuses_bad_arguments(cpu_backend):
    from fqss_amd import _lib
    from fqss_amd import kernels as K
    e, r = torch.randn(2, 3000), torch.randn(2, 3000)
    with pytest.raises(NotImplementedError, match="44100"):
        K.stoi(e, r, 44100)
    with pytest.raises(NotImplementedError, match="12000"):
        K.stoi(e, r, 12000)
    taps, up, down = K.stoi_taps(8000, "cpu")
    assert (taps.numel(), up, down) == (365, 5, 4) and K.stoi_taps(16000, "cpu")[0].numel() == 581
    assert K.stoi_taps(10000, "cpu")[0].tolist() == [1.0]
    need = _lib.query("fqss_stoi_ws_doubles", 2, 3000, 5, 4)
    Lp, NF = 3750, 28
    assert need == 2 * (2 * Lp + NF + (NF + 2) // 2 + 30 * (NF - 1) + 0)
    assert _lib.query("fqss_stoi_ws_doubles", 2, 9000, 1, 1) == 2 * (69 + 35 + 30 * 68 + 39)
    for args in ((0, 3000, 5, 4), (2, 0, 5, 4), (2, 3000, 10, 8), (2, 3000, 0, 4), (2, 3000, 5, -1)):
        assert _lib.query("fqss_stoi_ws_doubles", *args) == 0, args
    ws, d = torch.empty(need, dtype=torch.float64), torch.full((2,), 7.0, dtype=torch.float64)
    even = torch.ones(364, dtype=torch.float64)
    ok = [e.data_ptr(), r.data_ptr(), taps.data_ptr(), 365, ws.data_ptr(), need, d.data_ptr(), 2, 3000, 3000, 3000, 5, 4, None]
    bad = {"P < 1": {7: 0}, "L < 1": {8: 0}, "ld_e < L": {9: 2999}, "ld_r < L": {10: 2999}, "short workspace": {5: need - 1},
           "null est": {0: None}, "null ref": {1: None}, "null taps": {2: None}, "null ws": {4: None}, "null d": {6: None},
           "not reduced": {11: 10, 12: 8}, "up < 1": {11: 0}, "down < 1": {12: 0}, "even n_taps": {2: even.data_ptr(), 3: 364},
           "taps at 1 / 1": {11: 1, 12: 1}}
    for what, change in bad.items():
        args = list(ok)
        for i, v in change.items():
            args[i] = v
        with pytest.raises(_lib.FqssError, match="fqss_stoi"):
            _lib.call("fqss_stoi", *args)
    assert bool((d == 7.0).all())
    _lib.call("fqss_stoi", *ok)
    assert bool(((d > -1.0) & (d < 1.0)).all())
