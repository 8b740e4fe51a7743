"""fp64 NumPy checker of fqss_bss_eval (include/fqss.h) by a route the kernels do not take: no correlation sequences, no Toeplitz
structure, no Cholesky.  The lagged-reference matrix X of the zero-extended signals is built explicitly (L + T - 1 rows, one column per
(target, lag)); E_all and E_tgt are the energies of the estimate's least-squares projection on its columns (all of them / those of the
own target), taken from a QR factorisation of X.  A second route forms the normal equations X^T X, X^T e explicitly and solves them
with numpy.linalg.solve.  The spread of the two routes, per value in dB, is the checker's own uncertainty U."""
import numpy as np

FLOOR_DB = 1e-6      # fqss_sdr's gate
SPREAD_FACTOR = 1000.0      # the factor the STOI tests give their checker's spread
PANEL = 32      # columns per panel of the factorisation (kBssNB of csrc/bss_eval.hip)
SHAPES = [(S, T, L) for S in (1, 2, 3) for T, L in ((4, 500), (PANEL // 2, 1000), (PANEL // 3 + 1, 2500), (PANEL + 8, 1000))]


def normalise(x, zero_mean):
    x = np.asarray(x, np.float64)
    if zero_mean:
        x = x - x.mean(axis=-1, keepdims=True)
    return x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-6)


def lagged(ref, T):
    """[L + T - 1, S * T]: column (i, a) is ref_i delayed by a samples"""
    S, L = ref.shape
    X = np.zeros((L + T - 1, S * T))
    for i in range(S):
        for a in range(T):
            X[a:a + L, i * T + a] = ref[i]
    return X


def _ratio(num, den):
    if den <= 0.0 and num > 0.0:
        return np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(num / den)


def _energies(X, E, load, route):
    """e^T X (X^T X + load I)^-1 X^T e for every column e of E, from one factorisation of X"""
    n = X.shape[1]
    if route == "qr":      # least squares: the energy of the projection on the columns of [X; sqrt(load) I] is |Q^T [e; 0]|^2
        if load > 0.0:
            X, E = np.vstack([X, np.sqrt(load) * np.eye(n)]), np.vstack([E, np.zeros((n, E.shape[1]))])
        return np.sum((np.linalg.qr(X)[0].T @ E) ** 2, axis=0)
    D = X.T @ E
    return np.sum(D * np.linalg.solve(X.T @ X + load * np.eye(n), D), axis=0)


def bss_ref(est, ref, tgt=None, filter_length=512, zero_mean=False, load_diag=None, route="qr"):
    """[3, S]: SDR, SIR, SAR of fqss_bss_eval's statement"""
    S, L = ref.shape
    T = filter_length
    load = float(load_diag) if load_diag is not None and load_diag >= 0.0 else 0.0
    r, e = normalise(ref, zero_mean), normalise(est, zero_mean)
    X = lagged(r, T)
    E = np.vstack([e.T, np.zeros((T - 1, S))])      # the zero-extended estimates as columns
    own = [_energies(X[:, q * T:(q + 1) * T], E, load, route) for q in range(S)]
    every = _energies(X, E, load, route) if S > 1 else None
    out = np.empty((3, S))
    for j in range(S):
        q = j if tgt is None else int(tgt[j])
        E_j, E_tgt = float(e[j] @ e[j]), float(own[q][j])
        E_all = float(every[j]) if S > 1 else E_tgt
        out[:, j] = _ratio(E_tgt, E_j - E_tgt), _ratio(E_tgt, E_all - E_tgt), _ratio(E_all, E_j - E_all)
    return out


def bss_ref_with_spread(est, ref, **kw):
    """(the QR route's [3, S], U [3, S] = |QR route - normal-equations route| in dB, 0 where both are +inf)"""
    a, b = bss_ref(est, ref, route="qr", **kw), bss_ref(est, ref, route="normal", **kw)
    with np.errstate(invalid="ignore"):
        return a, np.where(a == b, 0.0, np.abs(a - b))


def check(got, want, U, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        diff = np.where(got == want, 0.0, np.abs(got - want))
    print(f"{what}: max |diff| = {np.nanmax(diff):.3e} dB, max U = {np.max(U):.3e} dB")
    assert np.all(diff <= np.maximum(FLOOR_DB, SPREAD_FACTOR * U)), (what, got, want, diff, U)


def make_case(S, L, seed):
    """targets: white noise through different short low-pass FIRs; estimate j: its target through a short FIR + 0.1 of the next target
    + white noise at -16 dB of it -- SIR near 20 dB, SAR near 15 dB.  fp32 (est, ref) [S, L]"""
    rs = np.random.RandomState(seed)
    lows = ([1.0, 0.7, 0.25], [1.0, 0.45, 0.1], [1.0, 0.2, 0.05])
    ref = np.stack([np.convolve(rs.randn(L + 2), lows[i], mode="valid") for i in range(S)]).astype(np.float32)
    est = np.empty_like(ref)
    for j in range(S):
        t = np.convolve(np.concatenate([np.zeros(2), ref[j].astype(np.float64)]), [0.9, 0.2, -0.1], mode="valid")
        other = 0.1 * ref[(j + 1) % S] if S > 1 else 0.0
        est[j] = (t + other + 0.16 * np.std(t) * rs.randn(L)).astype(np.float32)
    return est, ref
