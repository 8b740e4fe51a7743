"""fp64 checker of the signal-to-distortion ratio (fqss_sdr, include/fqss.h) and the inputs of its tests.

The definition is torchmetrics' SignalDistortionRatio with its defaults, which computes fast_bss_eval's `sdr`: both third party and
absent, so no fixture comes from them; the checker restates the published steps in NumPy by a route the kernels do not take
(correlations through numpy.fft, a dense LU solve of scipy.linalg.toeplitz(r)).  `sdr_ref(..., corr="direct" | "fft",
solver="lu" | "levinson")` are equivalent fp64 routes: their spread on the test grid is the checker's own noise, which the tolerances of
tests/test_sdr_cpu.py and tests/test_gpu_sdr.py are sized from."""
import numpy as np
import scipy.linalg

GATE_DB = 1e-6                      # |library - checker| in dB on every case (about 200 x the spread of the checker's routes, see test_sdr_cpu)
AR_COEFS = (0.0, 0.9, 0.99)
SNRS_DB = (0.0, 20.0, 60.0)
LENGTHS = (700, 2048, 6000)
FIR = (0.8, 0.35, -0.15)            # the 3-tap distortion filter of `estimate_of`


def ar1_noise(L, coef, seed):
    """white (coef = 0) or AR(1) low-pass noise x[t] = coef x[t - 1] + w[t], unit variance, fp32"""
    w = np.random.default_rng(seed).standard_normal(L + 200)
    if coef:
        x = np.empty_like(w)
        acc = 0.0
        for i, v in enumerate(w):
            acc = coef * acc + v
            x[i] = acc
        w = x
    w = w[200:]
    return (w / w.std()).astype(np.float32)


def estimate_of(target, snr_db, seed):
    """the target through the 3-tap FIR plus independent white noise `snr_db` below the filtered target, fp32"""
    t = target.astype(np.float64)
    f = np.convolve(t, FIR)[:len(t)]
    n = np.random.default_rng(seed).standard_normal(len(t))
    n *= np.sqrt((f ** 2).sum() / (n ** 2).sum()) * 10.0 ** (-snr_db / 20.0)
    return (f + n).astype(np.float32)


def grid_case(coef, snr_db, L):
    seed = 1000 * AR_COEFS.index(coef) + 100 * SNRS_DB.index(snr_db) + LENGTHS.index(L)
    t = ar1_noise(L, coef, seed)
    return estimate_of(t, snr_db, seed + 7919), t


GRID = [(c, s, L) for c in AR_COEFS for s in SNRS_DB for L in LENGTHS]


def _corr(t, p, F, how):
    """r[k] = sum_t t[t] t[t + k], b[k] = sum_t t[t] p[t + k], k < F, linear (absent terms where t + k >= L)"""
    L = len(t)
    if how == "fft":
        n = 1
        while n < 2 * L - 1:
            n *= 2
        T, P = np.fft.rfft(t, n), np.fft.rfft(p, n)
        r, b = np.fft.irfft(np.conj(T) * T, n)[:F], np.fft.irfft(np.conj(T) * P, n)[:F]
        if F > L:                                   # lags >= L of a length-n circular sum with n >= 2 L - 1 are the negative lags
            r, b = r.copy(), b.copy()
            r[L:] = 0.0
            b[L:] = 0.0
        if len(r) < F:
            r, b = np.pad(r, (0, F - len(r))), np.pad(b, (0, F - len(b)))
        return r, b
    r, b = np.zeros(F), np.zeros(F)
    for k in range(min(F, L)):
        r[k] = np.dot(t[:L - k], t[k:])
        b[k] = np.dot(t[:L - k], p[k:])
    return r, b


def sdr_ref(preds, target, filter_length=512, zero_mean=False, load_diag=None, corr="fft", solver="lu", want_cond=False):
    """SDR in dB of one pair, fp64; NaN (with numpy's warnings silenced) where the definition gives none"""
    p, t = np.asarray(preds, dtype=np.float64).copy(), np.asarray(target, dtype=np.float64).copy()
    if zero_mean:
        p -= p.mean()
        t -= t.mean()
    t /= max(np.sqrt((t * t).sum()), 1e-6)
    p /= max(np.sqrt((p * p).sum()), 1e-6)
    r, b = _corr(t, p, filter_length, corr)
    if load_diag is not None:
        r = r.copy()
        r[0] += load_diag
    with np.errstate(all="ignore"):
        try:
            sol = np.linalg.solve(scipy.linalg.toeplitz(r), b) if solver == "lu" else scipy.linalg.solve_toeplitz(r, b)
        except (np.linalg.LinAlgError, ValueError):
            return (float("nan"), float("inf")) if want_cond else float("nan")
        coh = float(np.dot(b, sol))
        db = 10.0 * np.log10(coh / (1.0 - coh))
    if want_cond:
        return float(db), float(np.linalg.cond(scipy.linalg.toeplitz(r)))
    return float(db)


def sdr_ref_rows(est, ref, **kw):
    return np.array([sdr_ref(e, r, **kw) for e, r in zip(np.asarray(est), np.asarray(ref))])


def closed_form_f1(preds, target):
    """filter_length = 1: coh = (t . p)^2 / (|t|^2 |p|^2), no solver involved"""
    p, t = np.asarray(preds, dtype=np.float64), np.asarray(target, dtype=np.float64)
    coh = np.dot(t, p) ** 2 / (np.dot(t, t) * np.dot(p, p))
    return float(10.0 * np.log10(coh / (1.0 - coh)))
