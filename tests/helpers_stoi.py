"""fp64 checker of the short-time objective intelligibility (fqss_stoi, include/fqss.h) and the inputs of its tests.

The definition is pystoi.stoi(clean, estimate, fs, extended=False), which the reference reaches through torchmetrics: third party and
absent, so no fixture comes from it; the checker restates the steps of the header comment in NumPy, from that statement and by routes
the kernels do not take (the resampler as a full convolution of the zero-stuffed signal, the silent-frame removal as an overlap-add
into a buffer, spectra through numpy.fft.rfft or, `dft="matrix"`, an explicit DFT-matrix product, segments as array slices).  The
spread of the two spectrum routes on the test grid is the checker's own noise, which the gate of tests/test_stoi_cpu.py and
tests/test_gpu_stoi.py is sized from."""
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -52
FS = 10000
N_FRAME, HOP, NFFT, N_BANDS, N_SEG = 256, 128, 512, 15, 30
DYN_RANGE_DB = 40.0
CLIP = 1.0 + 10.0 ** (15.0 / 20.0)
TOO_FEW = 1e-5                      # d when fewer than 30 spectral frames are left
RATES = (10000, 8000, 16000)
GRID_LENGTHS = {10000: 9000, 8000: 7200, 16000: 14400}      # 0.9 s
SNRS_DB = (20.0, 5.0, -5.0)


def gate(spread):
    """|library - checker| on d, from the spread S of the checker's two spectrum routes (the issue's rule: max(1e-12, 1000 S))"""
    return max(1e-12, 1000.0 * spread)


# ------------------------------------------------------------------------------------------------ the definition
def ratio(fs):
    f = Fraction(FS, int(fs))
    return f.numerator, f.denominator


def resample_window(p, q):
    """the taps of resample_oct before scipy's `* p`: kaiser x sinc, normalised to sum 1"""
    fc = 1.0 / (2.0 * max(p, q))
    half = int(np.ceil((60.0 - 8.0) / (28.714 * fc / 10.0)))
    t = np.arange(-half, half + 1)
    h = np.kaiser(2 * half + 1, 0.1102 * (60.0 - 8.7)) * (2.0 * p * fc * np.sinc(2.0 * fc * t))
    return h / h.sum()


def resample(x, p, q):
    """ceil(L p / q) samples of the zero-stuffed signal convolved with p * window, taken every q from the filter's centre"""
    x = np.asarray(x, dtype=np.float64)
    if p == q == 1:
        return x.copy()
    h = resample_window(p, q) * p
    half = (len(h) - 1) // 2
    up = np.zeros(len(x) * p)
    up[::p] = x
    full = np.convolve(up, h)
    n_out = -(-len(x) * p // q)
    idx = half + q * np.arange(n_out)
    full = np.pad(full, (0, max(0, idx[-1] + 1 - len(full))))
    return full[idx]


def window():
    return np.hanning(N_FRAME + 2)[1:-1]


def frame_starts(n):
    """0, 128, ... strictly below n - 256"""
    return np.arange(0, max(n - N_FRAME, 0), HOP)


def frame_energies_db(x):
    w = window()
    return np.array([20.0 * np.log10(np.linalg.norm(w * x[i:i + N_FRAME]) + EPS) for i in frame_starts(len(x))])


def remove_silent_frames(x, y):
    """(x, y) rebuilt from the frames whose clean energy is within 40 dB of the loudest, the mask, the margin in dB"""
    e = frame_energies_db(x)
    if len(e) == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0, dtype=bool), float("inf")
    keep = (e.max() - DYN_RANGE_DB - e) < 0
    margin = float(np.abs(e - (e.max() - DYN_RANGE_DB)).min())
    w, starts = window(), frame_starts(len(x))[keep]
    K = len(starts)
    xs, ys = np.zeros((K - 1) * HOP + N_FRAME), np.zeros((K - 1) * HOP + N_FRAME)
    for j, i in enumerate(starts):
        xs[j * HOP:j * HOP + N_FRAME] += w * x[i:i + N_FRAME]
        ys[j * HOP:j * HOP + N_FRAME] += w * y[i:i + N_FRAME]
    return xs, ys, keep, margin


_DFT = None


def spectra(x, dft="rfft"):
    """[257][T] complex spectra of the windowed frames, zero-padded to 512"""
    global _DFT
    w = window()
    starts = frame_starts(len(x))
    if len(starts) == 0:
        return np.zeros((NFFT // 2 + 1, 0), dtype=complex)
    frames = np.zeros((len(starts), NFFT))
    for j, i in enumerate(starts):
        frames[j, :N_FRAME] = w * x[i:i + N_FRAME]
    if dft == "rfft":
        return np.fft.rfft(frames, axis=1).T
    if _DFT is None:
        b, t = np.arange(NFFT // 2 + 1)[:, None], np.arange(NFFT)[None, :]
        _DFT = np.exp(-2j * np.pi * ((b * t) % NFFT) / NFFT)
    return _DFT @ frames.T


def band_edges():
    f = FS * np.arange(NFFT // 2 + 1) / NFFT
    k = np.arange(N_BANDS)
    lo = [int(np.argmin((f - v) ** 2)) for v in 150.0 * 2.0 ** ((2 * k - 1) / 6.0)]
    hi = [int(np.argmin((f - v) ** 2)) for v in 150.0 * 2.0 ** ((2 * k + 1) / 6.0)]
    return lo, hi


def third_octaves(spec):
    lo, hi = band_edges()
    p = np.abs(spec) ** 2
    return np.sqrt(np.stack([p[a:b].sum(axis=0) for a, b in zip(lo, hi)]))


def stoi_ref(est, ref, fs, dft="rfft", want_info=False):
    """d of one (estimate, clean) pair in fp64; with want_info also the kept-frame count and the mask margin in dB"""
    p, q = ratio(fs)
    x, y = resample(ref, p, q), resample(est, p, q)
    xs, ys, keep, margin = remove_silent_frames(x, y)
    K = int(keep.sum())
    x_tob, y_tob = third_octaves(spectra(xs, dft)), third_octaves(spectra(ys, dft))
    T = x_tob.shape[1]
    if T < N_SEG:
        d = TOO_FEW
    else:
        total = 0.0
        for m in range(N_SEG, T + 1):
            xseg, yseg = x_tob[:, m - N_SEG:m], y_tob[:, m - N_SEG:m]
            c = np.linalg.norm(xseg, axis=1, keepdims=True) / (np.linalg.norm(yseg, axis=1, keepdims=True) + EPS)
            yp = np.minimum(yseg * c, xseg * CLIP)
            xc, yc = xseg - xseg.mean(axis=1, keepdims=True), yp - yp.mean(axis=1, keepdims=True)
            xc = xc / (np.linalg.norm(xc, axis=1, keepdims=True) + EPS)
            yc = yc / (np.linalg.norm(yc, axis=1, keepdims=True) + EPS)
            total += float((xc * yc).sum())
        d = total / (N_BANDS * (T - N_SEG + 1))
    return (float(d), K, margin) if want_info else float(d)


def stoi_ref_rows(est, ref, fs, **kw):
    return np.array([stoi_ref(e, r, fs, **kw) for e, r in zip(np.asarray(est), np.asarray(ref))])


def taps(fs):
    """what the library is handed: p * window in fp64 ([1.0] at 10 kHz), and the reduced ratio"""
    p, q = ratio(fs)
    return (np.ones(1) if p == q == 1 else resample_window(p, q) * p), p, q


# ------------------------------------------------------------------------------------------------ inputs
def voiced(L, fs, seed, silence=((0.30, 0.48), (0.78, 0.92))):
    """a harmonic stack at 170 .. 3100 Hz under a ~3 Hz envelope plus 1e-5 of noise, fp32; the `silence` stretches (fractions of the
    length) are scaled by 1e-4"""
    rng = np.random.default_rng(seed)
    t = np.arange(L) / float(fs)
    f0 = 170.0 + 15.0 * rng.random()
    x = np.zeros(L)
    for h in range(1, 19):
        if f0 * h > 3100.0:
            break
        x += rng.uniform(0.3, 1.0) / h ** 0.5 * np.sin(2.0 * np.pi * f0 * h * t + 2.0 * np.pi * rng.random())
    x *= 0.55 + 0.45 * np.sin(2.0 * np.pi * 3.0 * t + rng.random())
    x = 0.1 * x / np.abs(x).max() + 1e-5 * rng.standard_normal(L)
    for a, b in silence:
        x[int(a * L):int(b * L)] *= 1e-4
    return x.astype(np.float32)


def noisy(ref, snr_db, seed):
    """the reference plus white noise `snr_db` below it (powers over the whole signal), fp32"""
    r = ref.astype(np.float64)
    n = np.random.default_rng(seed).standard_normal(len(r))
    n *= np.sqrt((r ** 2).sum() / (n ** 2).sum()) * 10.0 ** (-snr_db / 20.0)
    return (r + n).astype(np.float32)


def grid_case(fs, snr_db, L=None):
    L = GRID_LENGTHS[fs] if L is None else L
    seed = RATES.index(fs) * 10
    ref = voiced(L, fs, seed)
    return noisy(ref, snr_db, seed + 1 + SNRS_DB.index(snr_db)), ref


GRID = [(fs, snr) for fs in RATES for snr in SNRS_DB]
