"""An independent fp64 NumPy statement of the histogram-MSE activation observer (include/fqss.h, fqss_aq_hist / fqss_aq_mse_search) and the
test bodies tests/test_aq_mse_cpu.py (CPU backend) and tests/test_gpu_aq_mse.py (HIP kernels) share.  Histogram: np.histogram of the
fp64 image of x.  Merge and search: np.interp, vectorised over the candidates."""
import copy
import functools
import os

import numpy as np
import torch

BINS, N, MAX_M, MAX_ROWS = 512, 100, 65536, 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "act_mse.npz")


# ------------------------------------------------------------------------------------------------ the checker
def hist(x):
    """(counts int64 [512], edges fp64 [513]) of fp32 values: np.histogram on their fp64 image"""
    c, e = np.histogram(np.asarray(x, dtype=np.float32).reshape(-1).astype(np.float64), BINS)
    return c.astype(np.int64), e


def edges(lo, hi):
    lo, hi = np.float64(lo), np.float64(hi)
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    e = lo + np.arange(BINS + 1, dtype=np.float64) * ((hi - lo) / BINS)
    e[BINS] = hi
    return e


def merge(hists, rngs):
    """(M, b [M], vals [M - 1]) of rows (counts [512], (lo, hi)); rows whose range is not finite are void"""
    rows = [(np.asarray(h, dtype=np.int64), edges(r[0], r[1])) for h, r in zip(hists, rngs) if np.isfinite(r[0]) and np.isfinite(r[1])]
    assert rows
    bmin = min(e[0] for _, e in rows)
    bmax = max(e[-1] for _, e in rows)
    w = min((e[-1] - e[0]) / BINS for _, e in rows)
    M = np.ceil(((bmax + w) - bmin) / w)
    if not M <= MAX_M:
        w = (bmax - bmin) / (MAX_M - 1)
        M = min(np.ceil(((bmax + w) - bmin) / w), MAX_M)
    M = int(M)
    b = bmin + np.arange(M, dtype=np.float64) * w
    vals = None
    for h, e in rows:
        c = np.hstack([0, np.cumsum(h)]).astype(np.float64)
        d = np.diff(np.interp(b, e, c))
        vals = d if vals is None else vals + d
    return M, b, vals


def error_table(b, vals):
    """e [100, 100] over the left edges b[:-1] and their weights, and (delta, b0, bl)"""
    bl = b[:-1]
    b0, bk = bl[0], bl[-1]
    delta = 0.5 * (bk - b0) / N
    s = vals.sum()
    mx = (bk - delta * np.arange(N, dtype=np.float64))[:, None]
    e = np.empty((N, N))
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(N):
            mn = b0 + delta * i
            D = (mx - mn) / 255.0
            y = D * np.clip(np.rint((bl[None, :] - mn) / D), 0, 255) + mn
            e[i] = (np.square(bl[None, :] - y) * vals[None, :]).sum(1) / s
    return e, (delta, b0, bk)


def search(hists, rngs):
    """dict(M, b, vals, e, i, j, mn, mx, gap): the winner is the first strict minimum in (i, j) order; gap = (runner-up - min) / min"""
    M, b, vals = merge(hists, rngs)
    e, (delta, b0, bk) = error_table(b, vals)
    flat = np.where(np.isnan(e), np.inf, e).reshape(-1)
    k = int(np.argmin(flat))                       # first occurrence of the minimum
    srt = np.sort(flat)
    gap = (srt[1] - srt[0]) / srt[0] if srt[0] > 0 else np.inf
    i, j = divmod(k, N)
    return dict(M=M, b=b, vals=vals, e=e, i=i, j=j, mn=np.float32(b0 + delta * i), mx=np.float32(bk - delta * j), gap=gap,
                span=bk - b0)


# ------------------------------------------------------------------------------------------------ inputs
def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def obs_of(x, device):
    """the ordered-uint (min, max) words an OBSERVE launch leaves for x, as int32 [2] on the device"""
    def ordered(f):
        u = int(np.float32(f).view(np.uint32))
        return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)
    x = np.asarray(x, dtype=np.float32)
    words = np.array([ordered(x.min()), ordered(x.max())], dtype=np.uint32)
    return T(words.view(np.int32)).to(device)


def hist_inputs():
    """(name, x fp32 1-D, element offset of the view inside its 16-B aligned buffer): the sizes and contents of check 1"""
    g = np.random.default_rng(7)
    relu = g.standard_normal(1 << 16).astype(np.float32)
    relu[g.permutation(1 << 16)[:1 << 15]] = 0.0
    relu = np.maximum(relu, 0.0)
    base = (g.standard_normal(700) * 3).astype(np.float32)
    e = np.histogram(base.astype(np.float64), BINS)[1]
    on_edges = np.concatenate([e.astype(np.float32), [base.max()], np.nextafter(e.astype(np.float32), np.float32(np.inf))[:-1],
                               np.nextafter(e.astype(np.float32), np.float32(-np.inf))[1:], base]).astype(np.float32)
    on_edges = np.clip(on_edges, base.min(), base.max())
    return [("n1", np.array([1.25], dtype=np.float32), 0),
            ("n513", (g.standard_normal(513) * 2 + 0.3).astype(np.float32), 0),
            ("n4099", g.standard_normal(4099).astype(np.float32), 0),
            ("n4099_off1", g.standard_normal(4099).astype(np.float32), 1),
            ("relu_2^16", relu, 0),
            ("gauss_2^20", g.standard_normal(1 << 20).astype(np.float32), 0),
            ("edges", on_edges, 0),
            ("const", np.full(300, -2.5, dtype=np.float32), 3)]


def device_hist(K, x, device, offset=0):
    """(counts int64 [512], rng fp32 [2], obs words) of fqss_aq_hist on x, placed `offset` elements into an aligned buffer"""
    buf = torch.zeros(x.size + offset + 8, dtype=torch.float32, device=device)
    view = buf[offset:offset + x.size]
    view.copy_(T(x))
    assert view.data_ptr() % 16 == (4 * offset) % 16
    obs = obs_of(x, device)
    h = torch.zeros(BINS, dtype=torch.int32, device=device)
    r = torch.zeros(2, dtype=torch.float32, device=device)
    K.aq_hist(view, obs, h, r)
    return h.cpu().numpy().view(np.uint32).astype(np.int64), r.cpu().numpy(), obs.cpu().numpy().view(np.uint32)


def check_hist_case(K, name, x, offset, device):
    """check 1: counts == the checker's as integers, rng == (min, max) bit for bit, obs_ws reset"""
    got, r, obs = device_hist(K, x, device, offset)
    want, e = hist(x)
    assert np.array_equal(e, edges(x.min(), x.max())), name            # the statement's edges are np.histogram's (np.linspace)
    assert got.sum() == x.size and np.array_equal(got, want), (name, int(np.abs(got - want).sum()))
    assert r.view(np.uint32).tolist() == np.array([x.min(), x.max()], dtype=np.float32).view(np.uint32).tolist(), name
    assert obs.tolist() == [0xFFFFFFFF, 0], name
    return got


# (name, shape of the view, shape of the buffer it is cut from, element offset of the buffer): padded rows read in place
VIEW_CASES = [("7 x 4099 of ld 4112", (7, 4099), (7, 4112), 0),
              ("5 x 513 of ld 515, rows off 16-B alignment", (5, 513), (5, 515), 1),
              ("300 x 37 of ld 48", (300, 37), (300, 48), 0),
              ("2 x 3 x 100 of ld 112", (2, 3, 100), (2, 3, 112), 0),
              ("crop 2 x 3 x 5 x 8 of 2 x 3 x 7 x 8", (2, 3, 5, 8), (2, 3, 7, 8), 0)]


def check_hist_view_case(K, name, shape, full, offset, device):
    """a view with padded rows goes through fqss_aq_hist_rows in place (no gathering copy): counts == the checker's on the view's values;
    the padding holds 1e30, which no bin of the view's range may count"""
    from fqss_amd import _lib
    g = np.random.default_rng(len(name))
    x = (g.standard_normal(shape) * 1.5 + 0.2).astype(np.float32)
    n_full = int(np.prod(full))
    buf = torch.full((n_full + offset + 8,), 1e30, dtype=torch.float32, device=device)
    view = buf[offset:offset + n_full].view(*full)[tuple(slice(0, s) for s in shape)]
    view.copy_(T(x))
    assert not view.is_contiguous()
    obs = obs_of(x, device)
    h = torch.zeros(BINS, dtype=torch.int32, device=device)
    r = torch.zeros(2, dtype=torch.float32, device=device)
    calls, real = [], _lib.call
    _lib.call = lambda fn, *a: (calls.append(fn), real(fn, *a))[1]
    try:
        K.aq_hist(view, obs, h, r)
    finally:
        _lib.call = real
    assert calls == ["fqss_aq_hist_rows"], calls
    got = h.cpu().numpy().view(np.uint32).astype(np.int64)
    assert got.sum() == x.size and np.array_equal(got, hist(x)[0]), name
    assert r.cpu().numpy().tolist() == [float(x.min()), float(x.max())] and obs.cpu().numpy().view(np.uint32).tolist() == [0xFFFFFFFF, 0]


def rows_for(xs):
    """checker rows (counts, (lo, hi)) of a list of tensors"""
    return [hist(x)[0] for x in xs], [(np.float32(x.min()), np.float32(x.max())) for x in xs]


def merge_inputs():
    """(name, hists, rngs, expected M or None): the cases of check 2"""
    g = np.random.default_rng(11)
    one = [g.standard_normal(3000).astype(np.float32)]
    grow = [(g.standard_normal(1500) * (0.4 + 0.05 * t) + 0.01 * t).astype(np.float32) for t in range(50)]
    disjoint = [(g.standard_normal(2000) - 40).astype(np.float32), (g.standard_normal(2000) * 2 + 55).astype(np.float32)]
    cap = [(g.random(4000) * 1e-3).astype(np.float32), (g.random(4000) * 100 - 50).astype(np.float32)]
    out = [("T1", *rows_for(one), None), ("T50", *rows_for(grow), None), ("disjoint", *rows_for(disjoint), None)]
    h, r = rows_for(grow[:5])
    h.insert(2, np.zeros(BINS, dtype=np.int64))
    r.insert(2, (np.float32(np.nan), np.float32(np.nan)))
    out.append(("void_row", h, r, None))
    out.append(("cap", *rows_for(cap), MAX_M))
    return out


def device_search(K, hists, rngs, device):
    """fqss_aq_mse_search on rows -> (AqMseResult, qmin, qmax); the ranges start at the module's (-0.5, 0.5)"""
    h = T(np.stack([np.asarray(x, dtype=np.int64) for x in hists]).astype(np.uint32).view(np.int32)).to(device)
    r = T(np.array(rngs, dtype=np.float32).reshape(-1, 2)).to(device)
    qmin, qmax = torch.tensor([-0.5], device=device), torch.tensor([0.5], device=device)
    res = K.aq_mse_search(h, r, qmin, qmax, 8, want=True)
    return res, qmin, qmax


def check_merge_case(K, name, hists, rngs, want_M, device):
    """check 2: M equal, vals within 1e-12 * sum(vals) of the checker"""
    M, b, vals = merge(hists, rngs)
    assert want_M is None or M == want_M, (name, M)
    res, _, _ = device_search(K, hists, rngs, device)
    assert res.M == M, (name, res.M, M)
    got_b, got = res.b.cpu().numpy(), res.vals.cpu().numpy()
    np.testing.assert_allclose(got_b, b, rtol=1e-15, atol=0)
    worst = float(np.abs(got - vals).max())
    print(f"{name}: M {M}, max |vals - checker| {worst:.3g} of sum {vals.sum():.6g}")
    assert worst <= 1e-12 * vals.sum(), (name, worst)
    assert abs(got.sum() - sum(int(np.sum(h)) for h, r in zip(hists, rngs) if np.isfinite(r[0]))) <= 1e-9 * vals.sum()


@functools.lru_cache(maxsize=None)
def search_inputs():
    """(name, tensors, outliers on both sides): the inputs of check 3.  Seeds chosen on the CPU so that the checker's runner-up is more
    than 1e-6 relative above its minimum (asserted by the tests as a condition on the inputs)."""
    out = []
    g = np.random.default_rng(3)
    xs = []
    for t in range(6):
        x = g.standard_normal(4096) * (0.8 + 0.1 * t)
        x[5], x[77] = 60.0 + t, -(55.0 + 2 * t)                 # a far outlier on each side
        xs.append(x.astype(np.float32))
    out.append(("two_outliers", tuple(xs), True))
    g = np.random.default_rng(5)
    xs = [np.maximum(g.standard_normal(4096) * (1 + 0.2 * t), 0.0).astype(np.float32) for t in range(4)]
    for x in xs:
        x[9] = 40.0
    out.append(("relu_lo0", tuple(xs), False))
    g = np.random.default_rng(8)
    out.append(("plain", tuple((g.standard_normal(2048) * (1 + 0.5 * t) + 0.2).astype(np.float32) for t in range(3)), False))
    return tuple(out)


def check_search_case(K, name, xs, both, device):
    """check 3: the input condition (gap > 1e-6), (i*, j*) equal to the checker's and minimal at 1e-9, err_out at 1e-9, the ranges"""
    hists, rngs = rows_for(xs)
    ref = search(hists, rngs)
    assert ref["gap"] > 1e-6, (name, ref["gap"])                # a condition on the inputs
    res, qmin, qmax = device_search(K, hists, rngs, device)
    i, j = (int(v) for v in res.ij.cpu())
    best = float(res.best.cpu())
    e = ref["e"]
    print(f"{name}: M {ref['M']}, checker (i, j) = ({ref['i']}, {ref['j']}), gap {ref['gap']:.3g}; kernel ({i}, {j}), err {best:.12g} "
          f"vs {e[ref['i'], ref['j']]:.12g}")
    assert e[i, j] <= np.nanmin(e) * (1 + 1e-9), (name, i, j)
    assert abs(best - e[i, j]) <= 1e-9 * e[i, j], (name, best, e[i, j])
    assert (i, j) == (ref["i"], ref["j"]), (name, i, j, ref["i"], ref["j"])
    np.testing.assert_allclose(res.err.cpu().numpy(), e, rtol=1e-9)
    assert float(qmin.cpu()) == float(ref["mn"]) and float(qmax.cpu()) == float(ref["mx"]), name
    if both:
        assert i > 0 and j > 0, (name, i, j)                    # a kernel that returns the unshrunken range fails here
    if name == "relu_lo0":
        assert min(float(x.min()) for x in xs) == 0.0
    return ref


# ------------------------------------------------------------------------------------------------ the module
def mse_quantizer(device):
    from fqss_amd.quantization.qat import qat_quant as QQ
    return QQ.GradientActivationFakeQuantize_MSE(True).to(device)


def check_reference_fixture(K, device):
    """check 4: the module fed the 50 fixture tensors ends within 1e-5 of the span of the reference's own class's ranges; call 51 is
    bit-equal to a GradientActivationFakeQuantize holding the same ranges.  Returns the two differences in units of the span."""
    from fqss_amd.quantization.qat import qat_quant as QQ
    g = np.load(GOLDEN)
    xs, want = g["x"], g["range"]
    q = mse_quantizer(device)
    assert list(q.state_dict()) == ["min_range", "max_range"] and q.hist_n_bins == BINS and q.max_observations == 50
    assert tuple(q._hist.shape) == (50, BINS) and q._hist.dtype == torch.int32 and tuple(q._hist_rng.shape) == (50, 2)
    with torch.no_grad():
        for t in range(50):
            assert q.observing() and float(q.min_range.detach()) == -0.5 and float(q.max_range.detach()) == 0.5      # no EMA in this mode
            y = q(T(xs[t]).to(device))
            assert torch.equal(y.cpu(), T(xs[t]))                # the observer phase passes activations through
    assert not q.observing() and q.n_iter == 50 and q._hist is None and q._hist_rng is None
    ref = search(*rows_for(list(xs)))
    span = float(ref["b"][-1] - ref["b"][0])                     # bmax - bmin up to one bin
    d = [abs(float(q.min_range.detach()) - float(want[0])) / span, abs(float(q.max_range.detach()) - float(want[1])) / span]
    print(f"fixture: module ({float(q.min_range.detach())!r}, {float(q.max_range.detach())!r}), reference ({float(want[0])!r}, {float(want[1])!r}), "
          f"differences {d[0]:.3g} and {d[1]:.3g} of the span; checker (i, j) = ({ref['i']}, {ref['j']}), M {ref['M']}")
    assert max(d) <= 1e-5, d
    assert float(q.min_range.detach()) == float(ref["mn"]) and float(q.max_range.detach()) == float(ref["mx"])
    ema = QQ.GradientActivationFakeQuantize(True).to(device)
    ema.n_iter = ema.max_observations
    with torch.no_grad():
        ema.min_range.copy_(q.min_range)
        ema.max_range.copy_(q.max_range)
        x = T(xs[3].reshape(8, 256)).to(device)
        assert torch.equal(q(x), ema(x))
    return d


TINY = dict(n_spks=2, kernel_size=16, stride=8, n_filters=32, bn_chan=16, hid_chan=32, n_blocks=2, n_repeats=1)      # tiny_step.npz's model


def tiny_pair(device, act_observer=None, seed=0):
    from fqss_amd.quantization.qat.models.convtasnetq import ConvTasNetQ
    from fqss_amd.quantization.qat.models.load_model import quantize_model
    from fqss_amd.smoke import QCFG
    torch.manual_seed(seed)
    model = ConvTasNetQ(**TINY)
    fmodel = copy.deepcopy(model)
    cfg = dict(QCFG) if act_observer is None else dict(QCFG, act_observer=act_observer)
    return quantize_model(model, cfg).to(device).train(), fmodel.to(device).eval()


def act_quantizers(model):
    from fqss_amd.quantization.qat import qat_quant as QQ
    return [(n, m) for n, m in model.named_modules() if isinstance(m, QQ.GradientActivationFakeQuantize)]


class Spy:
    """records what the quantizers hand to kernels.aq_hist / aq_mse_search while it is installed (the scratch is freed by the search)"""

    def __init__(self, K):
        self.K, self.hist, self.search = K, K.aq_hist, K.aq_mse_search
        self.sizes, self.rows = {}, {}

    def __enter__(self):
        def aq_hist(x, obs, hrow, rrow):
            self.sizes.setdefault(hrow.data_ptr(), []).append(x.numel())
            return self.hist(x, obs, hrow, rrow)

        def aq_mse_search(hist, rng, qmin, qmax, n_bits=8, want=False):
            self.rows[qmin.data_ptr()] = (hist.cpu().numpy().view(np.uint32).astype(np.int64), rng.cpu().numpy(), hist.data_ptr())
            return self.search(hist, rng, qmin, qmax, n_bits, want)
        self.K.aq_hist, self.K.aq_mse_search = aq_hist, aq_mse_search
        return self

    def __exit__(self, *exc):
        self.K.aq_hist, self.K.aq_mse_search = self.hist, self.search


def check_model_observer_phase(K, device, x):
    """check 5, first half: 50 training forwards of the tiny ConvTasNetQ (batches of growing level) with minmax and with mse, one seed"""
    from fqss_amd.quantization.qat import qat_quant as QQ
    x = x.to(device)
    a, _ = tiny_pair(device, None)
    b, _ = tiny_pair(device, "mse")
    qa, qb = act_quantizers(a), act_quantizers(b)
    assert qa and [n for n, _ in qa] == [n for n, _ in qb]
    assert all(type(m) is QQ.GradientActivationFakeQuantize for _, m in qa)
    assert all(type(m) is QQ.GradientActivationFakeQuantize_MSE for _, m in qb)
    assert list(a.state_dict()) == list(b.state_dict())
    with Spy(K) as spy, torch.no_grad():
        for t in range(50):
            xt = x * (0.5 + 0.03 * t)
            ya, yb = a(xt), b(xt)
            assert torch.equal(ya, yb), t                       # the observer phase passes activations through un-quantized
    seen = 0
    for (n, m), (_, ma) in zip(qb, qa):
        assert m.n_iter == ma.n_iter, n
        if m.n_iter == 0:
            continue                                            # a quantizer the training forward never reaches
        seen += 1
        assert m.n_iter == 50 and not m.observing() and m._hist is None and m._hist_rng is None, n
        h, r, base = spy.rows[m.min_range.data_ptr()]
        assert h.shape == (50, BINS) and np.isfinite(r).all(), n
        rmin, rmax = np.float32(-0.5), np.float32(0.5)
        for t in range(50):                                     # r <- 0.9 r + 0.1 rng[t] in fp32: the EMA twin's arithmetic
            rmin = np.float32(0.9) * rmin + np.float32(0.1) * r[t, 0]
            rmax = np.float32(0.9) * rmax + np.float32(0.1) * r[t, 1]
        np.testing.assert_allclose([rmin, rmax], [float(ma.min_range.detach()), float(ma.max_range.detach())], rtol=1e-6, atol=0, err_msg=n)
        for t in range(50):                                     # each row sums to the element count of the tensor it observed
            assert spy.sizes[base + 4 * BINS * t] == [int(h[t].sum())], (n, t)
        assert len(set(h.sum(1).tolist())) == 1 and int(h[0].sum()) % x.shape[0] == 0, n      # one shape per quantizer, whole samples
        ref = search(list(h), [tuple(v) for v in r])
        assert ref["gap"] > 1e-6, (n, ref["gap"])               # a condition on the inputs, as in check 3: the winner is not a near-tie
        got = (float(m.min_range.detach()), float(m.max_range.detach()))
        assert got == (float(ref["mn"]), float(ref["mx"])), (n, got, ref["i"], ref["j"])
    assert seen >= 10, seen
    return a, b


def kd_run(act_observer, steps=60, B=2, samples=800, seed0=100):
    """`steps` KDTrainStep calls on a stream of synthetic batches, as the trainers drive it (maybe_capture before every step) ->
    (losses [steps], index of the step in front of which the graphs were recorded, final parameters, the model)"""
    from fqss_amd.data import synth_batch_2band
    from fqss_amd.runtime import KDTrainStep
    model, fmodel = tiny_pair("cuda", act_observer)
    step = KDTrainStep(model, fmodel, kd_lambda=0.1, lr=1e-3, clip=5.0)
    losses, captured = [], None
    for s in range(steps):
        x, tgt = synth_batch_2band(B, samples, seed0 + s, "cuda")
        step.maybe_capture(x, tgt)
        if captured is None and step._graphs is not None:
            captured = s
        losses.append(step(x, tgt)["loss"].reshape(()).clone())
    torch.cuda.synchronize()
    return torch.stack(losses).cpu().numpy(), captured, step.arena.flat_p.clone(), model
