"""Extended STOI (fqss_stoi_x) without a GPU: the fp64 checker of the statement in include/fqss.h -- the band matrices of
tests/helpers_stoi.py, every 15 x 30 segment normalised by rows, then by columns, a zero norm leaving zeros -- and the CPU backend against
it.  Gate: helpers_stoi.gate(S) = max(1e-12, 1000 S), S the spread of the checker's two spectrum routes (rfft / DFT matrix) on the grid.
Measured: S = 3.3e-16, CPU backend at most 7.8e-16 from the checker on the grid; on the frame-count inputs (d about 0.06) the routes differ
by 3.2e-14 and the backend is 3.6e-14 away.  The cases take `run(est, ref, fs) -> d`: tests/test_gpu_estoi.py runs them on the device."""
import functools

import numpy as np
import pytest
import torch

from tests import helpers_stoi as H


def unit(a, axis):
    a = a - a.mean(axis=axis, keepdims=True)
    n = np.linalg.norm(a, axis=axis, keepdims=True)
    return np.divide(a, n, out=np.zeros_like(a), where=n > 0)


def estoi_ref(est, ref, fs, dft="rfft"):
    """(d, segments) of one (estimate, clean) pair in fp64"""
    p, q = H.ratio(fs)
    xs, ys, _, margin = H.remove_silent_frames(H.resample(ref, p, q), H.resample(est, p, q))
    assert margin >= 0.1, margin          # a last-bit difference in log10 cannot flip a frame
    X, Y = H.third_octaves(H.spectra(xs, dft)), H.third_octaves(H.spectra(ys, dft))
    segs = [(unit(unit(X[:, m - 30:m], 1), 0) * unit(unit(Y[:, m - 30:m], 1), 0)).sum() / 30.0 for m in range(30, X.shape[1] + 1)]
    return (float(np.mean(segs)) if segs else H.TOO_FEW), len(segs)


def estoi_rows(est, ref, fs, **kw):
    return np.array([estoi_ref(e, r, fs, **kw)[0] for e, r in zip(est, ref)])


@functools.lru_cache(maxsize=None)
def grid(fs):
    """(est [3, L], ref [3, L], the checker's d [3], the gate) at 20 / 5 / -5 dB, computed once"""
    cases = [H.grid_case(fs, snr) for snr in H.SNRS_DB]
    est, ref = np.stack([e for e, _ in cases]), np.stack([r for _, r in cases])
    want = estoi_rows(est, ref, fs)
    S = np.abs(want - estoi_rows(est, ref, fs, dft="matrix")).max()
    print(f"fs = {fs}: checker d = {want}, spread S = {S:.3g}")
    return est, ref, want, H.gate(S)


def check(got, want, gate, what):
    err = np.abs(np.asarray(got) - np.asarray(want)).max()
    print(f"{what}: max |library - checker| = {err:.3g}, gate {gate:.3g}")
    assert np.isfinite(got).all() and err <= gate, (what, got, want)


def grid_case(run, fs):
    est, ref, want, gate = grid(fs)
    got = run(est, ref, fs)
    check(got, want, gate, f"grid fs = {fs}")
    assert got[0] > got[1] > got[2], got          # d falls as the noise rises


# 10 kHz, nothing silent: 256 + 128 n samples are n frames (the one ending at the last sample is dropped), one more sample n + 1;
# K frames are K - 1 spectral frames: 29 of them give 1e-5, 30 one segment, 31 two
FRAME_RULE = [(256 + 128 * 30, 0), (256 + 128 * 30 + 1, 1), (256 + 128 * 31, 1), (256 + 128 * 31 + 1, 2), (256 + 128 * 34, 4)]


def frame_case(run, L, segments):
    """the noisy estimate against the checker, est = ref is 1 within the gate, an all-zero estimate is exactly 0 (the zero-norm rule)"""
    ref = H.voiced(L, 10000, 77, silence=())
    est = H.noisy(ref, 5.0, 78)
    want, n = estoi_ref(est, ref, 10000)
    assert n == segments
    got = run(np.stack([est, ref, 0 * est]), np.stack([ref] * 3), 10000)
    if segments == 0:
        assert want == 1e-5 and (got == 1e-5).all(), got
    else:
        check(got[:2], [want, 1.0], grid(10000)[3], f"L = {L}: {segments} segments")
        assert got[2] == 0.0, got


@pytest.fixture()
def cpu_stoi():
    from fqss_amd import _lib
    from fqss_amd import kernels as K
    _lib.set_backend("cpu")
    yield lambda est, ref, fs, extended=True: K.stoi(torch.from_numpy(est), torch.from_numpy(ref), fs, extended=extended)
    _lib.set_backend("hip")


@pytest.mark.parametrize("fs", H.RATES)
def test_cpu_backend_estoi_on_the_grid_and_both_modes_in_one_call(cpu_stoi, fs):
    grid_case(lambda *a: cpu_stoi(*a).numpy(), fs)
    est, ref = grid(fs)[:2]
    both = cpu_stoi(est, ref, fs, "both")
    assert torch.equal(both[0], cpu_stoi(est, ref, fs, False)) and torch.equal(both[1], cpu_stoi(est, ref, fs))


@pytest.mark.parametrize("L,segments", FRAME_RULE)
def test_cpu_backend_estoi_frame_counts_and_zero_estimate(cpu_stoi, L, segments):
    frame_case(lambda *a: cpu_stoi(*a).numpy(), L, segments)
