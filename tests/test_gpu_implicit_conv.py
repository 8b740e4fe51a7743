"""The implicit-GEMM convolutions of HTDemucs (round 6) at kernel level against plain references: the pack / unpack moves
(fqss_halo_pack, fqss_phase_pack, fqss_phase_unpack) bit for bit against torch indexing, the four fqss_conv2_* entries against float64
sums of shifted-plane products on the contract include/fqss.h states (random planes everywhere, halo included, outputs inside guard
buffers), the plane-slack rule of conv2_impl, the layer paths (QL.conv_frames / QL.convtr_frames) against float64 autograd at the
shipped widths, the deterministic mode's fixed-point sums against float64, and the frozen teacher's regrouped-weight cache.

Tolerances follow test_pwconv_split_gemms_against_fp64: the normwise relative error against float64 (torch's own fp32 error printed
beside it), at most 3e-7 for three exact products per term (coded weights), 6e-7 for six products and for the data gradient, 1e-6 for
the split-K weight gradient, and elementwise |err| <= 4e-6 max|ref| so that one wrong column group cannot hide in a norm.  The implicit
GEMMs accumulate a whole reduction in one fp32 MFMA chain, so their rounding error grows as sqrt(K): measured on the MI355X at
(1.1 .. 1.7)e-8 sqrt(K) normwise for every case from K = 144 to K = 65520 (torch's fp32 GEMMs, with more partial sums: 1e-7 .. 6e-7).
The bounds therefore grow by sqrt(K / 768) past K = 768 (elementwise: past K = 3456).  A dropped bf16 piece is a relative error of
about 2^-17 = 7.6e-6 at any K: every bound, 5.5e-6 at K = 65520 included, stays below it."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
K = None
_lib = None
DEV = "cuda"
TOL = {"wq": 3e-7, "x3s": 6e-7, "dgrad": 6e-7, "wgrad": 1e-6}
ELEM = 4e-6


def tol(kind, K):
    """normwise bound of a K-long fp32 accumulation chain"""
    return TOL[kind] * math.sqrt(max(1.0, K / 768))


def elem(K):
    return ELEM * math.sqrt(max(1.0, K / 3456))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    global K, _lib
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from fqss_amd import _lib as lib
    from fqss_amd import kernels
    K, _lib = kernels, lib
    yield


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def r4(n):
    return (n + 3) // 4 * 4


def errs(a, ref):
    """(normwise relative, max abs / max |ref|) of a against a float64 reference"""
    d = a.double() - ref
    return float(d.norm() / ref.norm()), float(d.abs().max() / ref.abs().max())


class Guarded:
    """a float32 tensor of `shape` inside one buffer with G random floats on either side (16-B aligned: G % 4 == 0); `fill` (a value
    or a tensor) is written into the view, the whole buffer is remembered so that a write outside a region shows up"""
    G = 256

    def __init__(self, shape, seed, fill=None):
        n = math.prod(shape)
        self.buf = rnd(n + 2 * self.G, seed=seed).to(DEV)
        self.view = self.buf[self.G:self.G + n].view(*shape)
        if isinstance(fill, torch.Tensor):
            self.view.copy_(fill)
        elif fill is not None:
            self.view.fill_(fill)
        self.n = n
        self.before = self.buf.clone()

    def guards_intact(self):
        G, n = self.G, self.n
        return torch.equal(self.buf[:G], self.before[:G]) and torch.equal(self.buf[G + n:], self.before[G + n:])

    def unchanged(self, region_of):
        """region_of(t) -> the same region of the view and of its original contents"""
        old = self.before[self.G:self.G + self.n].view(self.view.shape)
        return torch.equal(region_of(self.view), region_of(old))


def same_bits(a, b):
    """equal element for element (the output was NaN-filled: a slot the kernel skipped keeps its NaN and fails the comparison)"""
    return a.shape == b.shape and not bool(torch.isnan(a).any()) and bool(torch.equal(a, b))


def strided_input(shape, layout, seed):
    """[B, C, H, W] signal in one of the layouts the pack kernels take: dense, a channel slice of a wider tensor (sc dense, sb wider),
    the rows of K.empty_act (row stride padded to 16 floats: sh > W) or the planes of K.empty_sig (H W padded to 16 floats)"""
    B, C, H, W = shape
    x = rnd(*shape, seed=seed)
    if layout == "contiguous":
        return x.to(DEV)
    if layout == "channel slice":
        wide = rnd(B, C + 3, H, W, seed=seed + 1).to(DEV)
        wide[:, 1:C + 1].copy_(x)
        return wide[:, 1:C + 1]
    if layout == "empty_act rows":
        t = K.empty_act((B, C, H, W), DEV)
        t.copy_(x)
        assert t.stride(2) > W
        return t
    t = K.empty_sig((B, C, H, W), DEV)
    t.copy_(x)
    return t


def sig_args(x):
    x2, sb, sc, sh = K._sig4(x)
    assert x2.data_ptr() == x.data_ptr(), "the layout under test must reach the kernel as is"
    return sb, sc, sh


def q0(r, s, p):
    return ((r + p) % s - p - r) // s       # (the numerator is a multiple of s: floor = the kernel's truncation)


# ----------------------------------------------------------------------------------------------------------------------------- pack / unpack
HALO_CASES = {
    "3x3 pad 1, W % 4 = 3, B = 2": ((2, 5, 9, 431), 1, 1, 0, "contiguous"),
    "pad (2, 0), W % 4 = 0, channel slice": ((2, 6, 7, 36), 2, 0, 4, "channel slice"),
    "pad (0, 2), W % 4 = 1, B = 3, empty_act rows": ((3, 4, 5, 37), 0, 2, 0, "empty_act rows"),
    "1-D row, pad 1, W % 4 = 2, empty_sig planes": ((2, 3, 1, 110), 0, 1, 8, "empty_sig planes"),
    "W = 3 < 4, pad (1, 2)": ((2, 3, 6, 3), 1, 2, 0, "contiguous"),
    "C = 1, plane 2^24 - 4 floats, Wp = 4092": ((1, 1, 4098, 4090), 1, 1, 0, "contiguous"),
}


@pytest.mark.parametrize("case", list(HALO_CASES))
def test_halo_pack_bit_exact(case):
    """fqss_halo_pack against F.pad: every one of the plane's floats written (NaN-filled planes), the halo and the slack behind the last
    row exactly 0, nothing written outside the planes.  The last case runs div_small (float-reciprocal division) over its whole range:
    4 i / Wp for 4 i up to 2^24 - 4 with a divisor that is not a power of two."""
    shape, ph, pw, extra, layout = HALO_CASES[case]
    B, C, H, W = shape
    x = strided_input(shape, layout, seed=1)
    sb, sc, sh = sig_args(x)
    Wp = r4(W + 2 * pw) + extra
    rows = H + 2 * ph
    plane = (1 << 24) - 4 if "2^24" in case else r4(rows * Wp + 13)
    assert rows * Wp <= plane < (1 << 24)
    out = Guarded((B, C, plane), seed=2, fill=float("nan"))
    _lib.call("fqss_halo_pack", x.data_ptr(), out.view.data_ptr(), B, C, H, W, sb, sc, sh, ph, pw, Wp, plane, None)
    torch.cuda.synchronize()
    ref = F.pad(x, (pw, Wp - W - pw, ph, ph)).reshape(B, C, rows * Wp)
    ref = F.pad(ref, (0, plane - rows * Wp))
    assert same_bits(out.view, ref), case
    halo = torch.ones(rows, Wp, dtype=torch.bool, device=DEV)
    halo[ph:ph + H, pw:pw + W] = False
    assert bool((out.view[:, :, :rows * Wp].view(B, C, rows, Wp)[:, :, halo] == 0).all()) and bool((out.view[:, :, rows * Wp:] == 0).all())
    assert out.guards_intact()
    if "2^24" not in case:          # the wrapper: its own buffer, the same values
        assert torch.equal(K.halo_pack(x, ph, pw, Wp, plane), ref)


def phase_pack_ref(x, s, p, axis, Wp, plane):
    B, C, H, W = x.shape
    idx = torch.arange(plane, device=x.device)
    out = torch.zeros(B, C, s, plane, device=x.device)
    for r in range(s):
        if axis == 0:
            m, w = idx // Wp, idx % Wp
            h = s * (m + q0(r, s, p)) + r
            ok = (h >= 0) & (h < H) & (w < W)
            out[:, :, r, ok] = x[:, :, h[ok], w[ok]]
        else:
            col = s * (idx + q0(r, s, p)) + r
            ok = (col >= 0) & (col < W)
            out[:, :, r, ok] = x[:, :, 0, col[ok]]
    return out.view(B, C * s, plane)


PHASE_CASES = {
    # name: (axis, k, s, p, shape, layout)
    "k8 s4 p0, 1-D, W % 4 = 0": (1, 8, 4, 0, (2, 3, 1, 1336), "contiguous"),
    "k8 s4 p1, 1-D, W % 4 = 1, channel slice": (1, 8, 4, 1, (2, 3, 1, 1333), "channel slice"),
    "k8 s4 p2, 1-D, W % 4 = 2, empty_act rows": (1, 8, 4, 2, (1, 4, 1, 1334), "empty_act rows"),
    "k8 s4 p3, 1-D, W % 4 = 3, B = 3": (1, 8, 4, 3, (3, 2, 1, 1335), "contiguous"),
    "k6 s2 p1, 1-D": (1, 6, 2, 1, (2, 3, 1, 801), "contiguous"),
    "k4 s2 p1, 1-D, empty_sig planes": (1, 4, 2, 1, (2, 3, 1, 802), "empty_sig planes"),
    "(8, 1) s4 p2, W % 4 = 1, channel slice": (0, 8, 4, 2, (2, 3, 64, 37), "channel slice"),
    "(8, 1) s4 p1, W = 3 < 4": (0, 8, 4, 1, (2, 2, 33, 3), "contiguous"),
    "(8, 1) s4 p3, 431 columns": (0, 8, 4, 3, (1, 2, 128, 431), "contiguous"),
    "(8, 1) s4 p0, W % 4 = 0, empty_act rows": (0, 8, 4, 0, (2, 3, 16, 36), "empty_act rows"),
    "(6, 1) s2 p1, W % 4 = 2, B = 3": (0, 6, 2, 1, (3, 2, 31, 6), "empty_sig planes"),
    "(4, 1) s2 p1, W % 4 = 2": (0, 4, 2, 1, (2, 3, 20, 10), "contiguous"),
}


@pytest.mark.parametrize("case", list(PHASE_CASES))
def test_phase_pack_bit_exact(case):
    """fqss_phase_pack against the explicit gather xp[b][c s + r][m Wp + w] = x[b][c][s (m + q0(r)) + r][w] (axis 0; axis 1:
    xp[b][c s + r][j] = x[b][c][0][s (j + q0(r)) + r]), zero outside the signal, on the planes of the layer's own PhasePlan:
    NaN-filled planes, nothing written outside them"""
    axis, k, s, p, shape, layout = PHASE_CASES[case]
    B, C, H, W = shape
    geom = K.ConvGeom((k, 1), (s, 1), (p, 0)) if axis == 0 else K.ConvGeom((1, k), (1, s), (0, p))
    assert K.PhasePlan.serves(H, W, geom)
    pp = K.PhasePlan(H, W, geom)
    Wp, plane = pp.inner.Wp, pp.inner.plane_x
    x = strided_input(shape, layout, seed=3)
    sb, sc, sh = sig_args(x)
    out = Guarded((B, C * s, plane), seed=4, fill=float("nan"))
    _lib.call("fqss_phase_pack", x.data_ptr(), out.view.data_ptr(), B, C, H, W, sb, sc, sh, axis, s, p, Wp, plane, None)
    torch.cuda.synchronize()
    ref = phase_pack_ref(x, s, p, axis, Wp, plane)
    assert same_bits(out.view, ref), case
    assert out.guards_intact()
    assert torch.equal(K.phase_pack(x, pp), ref)


def phase_unpack_ref(gy, C, s, p, axis, H, W, Hy, Wp, off, bias):
    B, plane = gy.shape[0], gy.shape[-1]
    g = gy.view(B, C, s, plane)
    pos = torch.arange(H if axis == 0 else W, device=gy.device) + off
    r = pos % s
    m = pos // s - torch.tensor([q0(i, s, p) for i in range(s)], device=gy.device)[r]
    ok = (m >= 0) & (m < Hy)
    mc = m.clamp(0, Hy - 1)
    if axis == 0:
        flat = (mc[:, None] * Wp + torch.arange(W, device=gy.device)[None, :])      # [H, W]
        v = g[:, :, r[:, None].expand(H, W), flat]                                  # [B, C, H, W]
        v = torch.where(ok[:, None], v, torch.zeros((), device=gy.device))
    else:
        v = g[:, :, r, mc]                                                           # [B, C, W]
        v = torch.where(ok, v, torch.zeros((), device=gy.device)).unsqueeze(2)
    return v + (bias.view(1, C, 1, 1) if bias is not None else 0.0)


UNPACK_CASES = {
    # name: (axis, s, p, B, C, H, W, Hy, off, bias)
    "(8, 1) s4 p2, 431 columns (unpack4), window from row 2, bias": (0, 4, 2, 2, 3, 128, 431, 33, 2, True),
    "(8, 1) s4 p0, W = 5 (unpack), no bias": (0, 4, 0, 2, 3, 40, 5, 11, 0, False),
    "(4, 1) s2 p1, W = 8 (unpack4), B = 3, bias": (0, 2, 1, 3, 2, 21, 8, 12, 0, True),
    "(8, 1) s4 p3, W = 9 (unpack4, W % 4 = 1), window from row 3": (0, 4, 3, 1, 2, 30, 9, 10, 3, False),
    "k8 s4 p0, 1-D 1322 (unpack4), window from 3, bias": (1, 4, 0, 2, 3, 1, 1322, 332, 3, True),
    "k6 s2 p1, 1-D W = 7 (unpack), window from 1, bias": (1, 2, 1, 2, 3, 1, 7, 5, 1, True),
    "k8 s4 p2, 1-D W = 1333 (unpack4), no bias": (1, 4, 2, 1, 2, 1, 1333, 335, 0, False),
    "(8, 1) s4 p2, W = 7, C = 1: H W = 2^24 - 1 (unpack: div_small over its range)": (0, 4, 2, 1, 1, 2396745, 7, 599188, 0, True),
}


@pytest.mark.parametrize("case", list(UNPACK_CASES))
def test_phase_unpack_bit_exact(case):
    """fqss_phase_unpack against the explicit inverse gather (+ bias) into a destination whose rows are wider than the signal (sh > W):
    every signal element written (NaN-filled destination), its padding columns and everything around it untouched; both kernel forms
    (k_phase_unpack for W < 8, k_phase_unpack4 for W >= 8), windows that start `off` positions in, bias present and absent.  The source
    planes hold random values beyond the Hy live rows: a read past them shows up."""
    axis, s, p, B, C, H, W, Hy, off, use_bias = UNPACK_CASES[case]
    Wp = r4(W) + (4 if axis == 0 and W < 100 else 0)
    if axis == 1:
        Wp = r4(max(Hy, 8))
    plane = r4(Hy * Wp + 5) if axis == 0 else Wp
    gy = rnd(B, C * s, plane, seed=5).to(DEV)
    bias = rnd(C, seed=6).to(DEV) if use_bias else None
    Wd = W + 5                                            # destination rows: W floats of signal + 5 of padding (sh > W)
    dst = Guarded((B, C, H, Wd), seed=7, fill=float("nan"))
    view = dst.view[..., :W]
    sb, sc, sh = view.stride(0), view.stride(1), view.stride(2)
    if axis == 1:
        sh = Wd
    _lib.call("fqss_phase_unpack", gy.data_ptr(), view.data_ptr(), B, C, H, W, sb, sc, sh, axis, s, p, Hy, Wp, plane, off,
              None if bias is None else bias.data_ptr(), None)
    torch.cuda.synchronize()
    ref = phase_unpack_ref(gy, C, s, p, axis, H, W, Hy, Wp, off, bias)
    assert same_bits(view.contiguous(), ref), case
    assert bool(torch.isnan(dst.view[..., W:]).all()), "padding columns of the destination were written"
    assert dst.guards_intact()


# ----------------------------------------------------------------------------------------------------------------------------- fqss_conv2_*
def flat_conv_ref(xp, Wm, taps, shifts, N, bias=None):
    """z[b][m][n] = bias[m] + sum_{c, t} Wm[m][c taps + t] xp[b][c][n + shifts[t]], n < N (the contract of include/fqss.h)"""
    B, Cr, _ = xp.shape
    M = Wm.shape[0]
    W3 = Wm.view(M, Cr, taps)
    z = torch.zeros(B, M, N, dtype=xp.dtype, device=xp.device)
    for t, sft in enumerate(shifts):
        z += torch.einsum("mc,bcn->bmn", W3[:, :, t], xp[:, :, sft:sft + N])
    if bias is not None:
        z += bias.view(1, M, 1).to(z.dtype)
    return z


def wgrad_ref(gzp, xp, taps, kw, row_step, col_step, off):
    """gw[co][ci taps + t] = sum_{b, m < plane_g} gzp[b][co][m] xp[b][ci][m + sft(t) - off], zero outside [0, plane_x)"""
    B, Co, Pg = gzp.shape
    Ci, Px = xp.shape[1], xp.shape[2]
    gw = torch.zeros(Co, Ci, taps, dtype=gzp.dtype, device=gzp.device)
    for t in range(taps):
        sft = (t // kw) * row_step + (t % kw) * col_step - off
        lo, hi = max(0, -sft), min(Pg, Px - sft)
        if hi > lo:
            gw[:, :, t] = torch.einsum("bom,bcm->oc", gzp[:, :, lo:hi], xp[:, :, lo + sft:hi + sft])
    return gw.view(Co, Ci * taps)


def tap_shifts(taps, kw, base, row_step, col_step):
    return [base + (t // kw) * row_step + (t % kw) * col_step for t in range(taps)]


def int8_weight(M, Kr, seed):
    g = torch.Generator().manual_seed(seed)
    wi = torch.randint(-127, 128, (M, Kr), generator=g, dtype=torch.int8)
    return wi


def run_conv2(entry, xp, A, dw, bias, B, Cr, M, taps, kw, base, row_step, col_step, N, plane_in, plane_out, z):
    """one fqss_conv2_* forward-form entry through the C ABI; xp [B][Cr][plane_in], z [B][M][plane_out]"""
    p = lambda t: None if t is None else t.data_ptr()
    if entry == "fwd_wq":
        _lib.call("fqss_conv2_fwd_wq", p(xp), p(A), p(dw), p(bias), p(z), B, Cr, M, taps, kw, base, row_step, col_step, N, plane_in, plane_out, None)
    elif entry == "bwd_x_wq":          # (Cr = the gradient's channels = the conv's Co; M = its Ci; dw [Cr] scales the reduction rows)
        _lib.call("fqss_conv2_bwd_x_wq", p(xp), p(A), p(dw), p(z), B, M, Cr, taps, kw, base, row_step, col_step, N, plane_in, plane_out, None)
    else:
        _lib.call("fqss_conv2_fwd_x3s", p(xp), p(A), p(bias), p(z), B, Cr, M, taps, kw, base, row_step, col_step, N, plane_in, plane_out, None)


def conv2_operands(entry, Cr, M, taps, seed):
    """(A as the kernel takes it, dw, bias, the float64 matrix Wm [M][Cr taps] of the sum, bias in float64)"""
    Kr = Cr * taps
    if entry in ("fwd_wq", "bwd_x_wq"):
        wi = int8_weight(M, Kr, seed).to(DEV)
        nd = Cr if entry == "bwd_x_wq" else M
        dw = ((0.5 + torch.rand(nd, generator=torch.Generator().manual_seed(seed + 1))) / (127 * math.sqrt(Kr))).to(DEV)
        if entry == "fwd_wq":
            Wm = wi.double() * dw.double()[:, None]
        else:
            Wm = (wi.double().view(M, Cr, taps) * dw.double().view(1, Cr, 1)).view(M, Kr)
        A = wi
    else:
        dw = None
        A = rnd(M, Kr, seed=seed, scale=Kr ** -0.5).to(DEV)
        Wm = A.double()
    bias = rnd(M, seed=seed + 2).to(DEV) if entry in ("fwd_wq", "fwd_x3s") else None
    return A, dw, bias, Wm


# name: (B, Ci, Co, (kh, kw), (ph, pw), (dh, dw), H, W) -- the shipped shapes are the cfg-5 model's at 10 s (HTDemucsQ, 4 stems, 44.1 kHz):
# its decoder.0 `rewrite`, the tdecoder.3 `rewrite` on the first time encoder's 110250 samples, and the inner stride-1 convolution of
# encoder.2 (Conv2d(96, 192, (8, 1), (4, 1), (2, 0)) on 128 x 431: T = 2 taps over 4 x 96 phase planes of 33 rows)
CONV_CASES = {
    "decoder.0 rewrite Conv2d(384, 768, 3, 1, 1) on 8 x 431 (N % 8 = 0)": (1, 384, 768, (3, 3), (1, 1), (1, 1), 8, 431),
    "tdecoder.3 rewrite Conv1d(48, 96, 3, 1, 1) on 110250 (N % 8 = 4)": (1, 48, 96, (1, 3), (0, 1), (1, 1), 1, 110250),
    "encoder.2 phase planes: 384 -> 192, (2, 1) taps on 33 x 431": (1, 384, 192, (2, 1), (0, 0), (1, 1), 33, 431),
    "K = 65520: Ci 7280, 3 x 3, Co 40": (1, 7280, 40, (3, 3), (1, 1), (1, 1), 3, 5),
    "Co 130, (3, 1) kernel, B = 3": (3, 32, 130, (3, 1), (1, 0), (1, 1), 9, 37),
    "Co 1024: the coded data gradient stages 1024 delta_w": (1, 64, 1024, (3, 3), (1, 1), (1, 1), 6, 29),
    "taps = 1": (2, 64, 48, (1, 1), (0, 0), (1, 1), 5, 23),
    "3 x 3 dilation 2 pad 2, B = 2": (2, 32, 80, (3, 3), (2, 2), (2, 2), 11, 29),
}


def _entries(Ci, Co, taps):
    """the entries whose host checks admit the case: reductions Ci taps (forward) / Co taps (data gradient) % 16 for coded weights,
    % 4 for float ones; at most 1024 reduction channels for the coded data gradient"""
    out = []
    if (Ci * taps) % 4 == 0:
        out.append("fwd_x3s")
    if (Ci * taps) % 16 == 0:
        out.append("fwd_wq")
    if (Co * taps) % 4 == 0:
        out.append("dgrad_x3s")
    if (Co * taps) % 16 == 0 and Co <= 1024:
        out.append("bwd_x_wq")
    return out + ["bwd_w"]


CONV_PARAMS = [(c, e) for c, v in CONV_CASES.items() for e in _entries(v[1], v[2], v[3][0] * v[3][1])]


def test_conv2_cases_cover_the_shipped_entries():
    shipped = [c for c in CONV_CASES if c.startswith(("decoder.0", "tdecoder.3", "encoder.2"))]
    for c in shipped:
        assert {e for cc, e in CONV_PARAMS if cc == c} == {"fwd_x3s", "fwd_wq", "dgrad_x3s", "bwd_x_wq", "bwd_w"}, c
    assert ("Co 1024: the coded data gradient stages 1024 delta_w", "bwd_x_wq") in CONV_PARAMS
    enc = K.PhasePlan(128, 431, K.ConvGeom((8, 1), (4, 1), (2, 0)))
    assert (enc.inner.H, enc.inner.W, enc.T, enc.s) == (33, 431, 2, 4)


@pytest.mark.parametrize("case,entry", CONV_PARAMS)
def test_conv2_against_fp64(case, entry):
    """fqss_conv2_* on the geometry a HaloPlan gives the case (forward: base 0, steps (dh Wp, dw) over N = Ho Wp; data gradient:
    negative steps from base (kh-1) dh Wp + (kw-1) dw over N = H Wp on the plane_g planes; weight gradient: off = phg Wp + pwg), with
    random values everywhere in the planes -- halo included -- so that each of the N outputs is a sum of live products.  The output is
    a [B][M][plane_out] region inside a guard buffer with plane_out = roundup4(N) + 12: the N outputs against float64, nothing past
    column roundup4(N) of any plane and nothing outside the region changed.  fqss_conv2_bwd_w ADDS into a pre-filled gw.
    Measured on one MI355X (normwise; torch fp32 beside it): decoder.0 rewrite x3s 6.5e-7 (2.5e-7), wq 2.9e-7 (1.8e-7), dgrad x3s 1.35e-6
    (5.0e-7), bwd_x_wq 8.4e-7 (5.0e-7), bwd_w 5.1e-7 (1.2e-6); tdecoder.3 rewrite 1.3e-7 / 6.4e-8 / 2.6e-7 / 1.6e-7 / 5.7e-7; encoder.2
    3.1e-7 / 1.4e-7 / 3.0e-7 / 1.9e-7 / 3.4e-7; K = 65520 x3s 4.0e-6 (5.7e-7), wq 1.8e-6 (4.6e-7); Co 1024 dgrad x3s 1.6e-6 (3.0e-7),
    bwd_x_wq 9.9e-7 (3.0e-7); every other case <= 4.1e-7.  Each sits at 1.3x .. 5x below its bound."""
    B, Ci, Co, (kh, kw), (ph, pw), (dh, dw_), H, W = CONV_CASES[case]
    plan = K.HaloPlan(H, W, K.ConvGeom((kh, kw), (1, 1), (ph, pw), (dh, dw_)))
    taps, Wp = plan.taps, plan.Wp
    seed = sum(map(ord, case + entry)) % 1000
    if entry == "bwd_w":
        gzp = rnd(B, Co, plan.plane_g, seed=seed).to(DEV)
        xp = rnd(B, Ci, plan.plane_x, seed=seed + 1).to(DEV)
        off = plan.phg * Wp + plan.pwg
        gw0 = rnd(Co, Ci * taps, seed=seed + 2)
        gw = Guarded((Co, Ci * taps), seed=seed + 3, fill=gw0)
        _lib.call("fqss_conv2_bwd_w", gzp.data_ptr(), xp.data_ptr(), gw.view.data_ptr(), B, Ci, Co, taps, kw, dh * Wp, dw_, off,
                  plan.plane_g, plan.plane_x, None)
        torch.cuda.synchronize()
        ref = wgrad_ref(gzp.double(), xp.double(), taps, kw, dh * Wp, dw_, off)
        e, em = errs(gw.view.double() - gw0.to(DEV).double(), ref)
        et, _ = errs(wgrad_ref(gzp, xp, taps, kw, dh * Wp, dw_, off), ref)
        print(f"{case} / {entry}: {e:.2e} (elementwise {em:.2e}); torch fp32 {et:.2e}")
        assert gw.guards_intact()
        assert e <= TOL["wgrad"] and em <= ELEM, (e, em)
        return
    if entry in ("fwd_x3s", "fwd_wq"):
        Cr, M, base, rs, cs, N, plane_in = Ci, Co, 0, dh * Wp, dw_, plan.Ho * Wp, plan.plane_x
    else:
        Cr, M, N, plane_in = Co, Ci, plan.H * Wp, plan.plane_g
        base, rs, cs = (kh - 1) * dh * Wp + (kw - 1) * dw_, -dh * Wp, -dw_
    kern = "x3s" if entry == "dgrad_x3s" else entry
    xp = rnd(B, Cr, plane_in, seed=seed).to(DEV)
    A, dwv, bias, Wm = conv2_operands("fwd_x3s" if kern == "x3s" else kern, Cr, M, taps, seed + 1)
    if entry == "dgrad_x3s":
        bias = None                      # (a data gradient has none)
    plane_out = r4(N) + 12
    z = Guarded((B, M, plane_out), seed=seed + 2)
    run_conv2("fwd_x3s" if kern == "x3s" else kern, xp, A, dwv, bias, B, Cr, M, taps, kw, base, rs, cs, N, plane_in, plane_out, z.view)
    torch.cuda.synchronize()
    sh = tap_shifts(taps, kw, base, rs, cs)
    ref = flat_conv_ref(xp.double(), Wm, taps, sh, N, None if bias is None else bias.double())
    e, em = errs(z.view[:, :, :N], ref)
    et, _ = errs(flat_conv_ref(xp, Wm.float(), taps, sh, N, bias), ref)
    print(f"{case} / {entry} (N = {N}, K = {Cr * taps}): {e:.2e} (elementwise {em:.2e}); torch fp32 {et:.2e}")
    assert z.guards_intact() and z.unchanged(lambda t: t[:, :, r4(N):]), "write past column roundup4(N) or outside the output"
    bound = tol("wq" if entry == "fwd_wq" else "dgrad" if entry in ("dgrad_x3s", "bwd_x_wq") else "x3s", Cr * taps)
    assert e <= bound and em <= elem(Cr * taps), (e, bound, em, elem(Cr * taps))


def _slack_geometry(N):
    """a 3 x 3 tap map on rows of Wp = 12 floats: forward shifts 0 .. 2 Wp + 2"""
    Wp = 12
    return dict(taps=9, kw=3, base=0, rs=Wp, cs=1, N=N), 2 * Wp + 2


@pytest.mark.parametrize("n_mod8", [1, 2, 3])
@pytest.mark.parametrize("entry", ["fwd_x3s", "fwd_wq", "bwd_x_wq"])
def test_conv2_any_n_through_the_c_abi(entry, n_mod8):
    """the C ABI does not require N % 4 == 0 (HaloPlan always gives it): N % 8 = 1, 2, 3 on planes with room to spare -- the N outputs
    against float64, columns [N, roundup4(N)) may take the epilogue's 4-wide store, nothing past them changes"""
    N = 8 * 9 + n_mod8
    geo, smax = _slack_geometry(N)
    Cr, M, B = 16, 40, 2
    plane_in = r4(N + smax + 8) + 16
    xp = rnd(B, Cr, plane_in, seed=n_mod8).to(DEV)
    A, dwv, bias, Wm = conv2_operands(entry, Cr, M, geo["taps"], seed=10 + n_mod8)
    plane_out = r4(N) + 8
    z = Guarded((B, M, plane_out), seed=3)
    run_conv2(entry, xp, A, dwv, bias, B, Cr, M, geo["taps"], geo["kw"], geo["base"], geo["rs"], geo["cs"], N, plane_in, plane_out, z.view)
    torch.cuda.synchronize()
    ref = flat_conv_ref(xp.double(), Wm, geo["taps"], tap_shifts(geo["taps"], geo["kw"], geo["base"], geo["rs"], geo["cs"]), N,
                        None if bias is None else bias.double())
    e, em = errs(z.view[:, :, :N], ref)
    print(f"{entry}, N = {N}: {e:.2e} (elementwise {em:.2e})")
    assert z.guards_intact() and z.unchanged(lambda t: t[:, :, r4(N):])
    assert e <= TOL["x3s"] and em <= ELEM, (e, em)


@pytest.mark.parametrize("n_mod8", [1, 4])
@pytest.mark.parametrize("entry", ["fwd_x3s", "fwd_wq", "bwd_x_wq"])
def test_conv2_plane_slack_contract(entry, n_mod8):
    """include/fqss.h: a packed plane must hold ((N - 1) / 8) 8 + 8 floats behind the largest tap shift -- the implicit loader moves
    8-column groups and clamps a group's start to the last one that fits, so a plane shorter than that fed the last live group from
    shifted columns without an error.  At the smallest plane the old check admitted (N + smax, rounded up to 4 floats) the call must be
    right or refused with FqssError; at the smallest plane the rule admits it must be right; at the largest plane below that minimum
    that the alignment rule (plane % 4 == 0) still admits, it must be refused.  Every plane is allocated whole: the loads stay inside
    it whatever the check decides."""
    N = 8 * 11 + n_mod8
    geo, smax = _slack_geometry(N)
    Cr, M, B = 16, 40, 1
    p_old = r4(N + smax)
    p_min = r4((N - 1) // 8 * 8 + 8 + smax)
    assert p_old < p_min
    A, dwv, bias, Wm = conv2_operands(entry, Cr, M, geo["taps"], seed=20 + n_mod8)
    sh = tap_shifts(geo["taps"], geo["kw"], geo["base"], geo["rs"], geo["cs"])
    outcome = {}
    for plane_in in (p_old, p_min - 4, p_min):
        xp = rnd(B, Cr, plane_in, seed=plane_in).to(DEV)
        z = Guarded((B, M, r4(N)), seed=5)
        try:
            run_conv2(entry, xp, A, dwv, bias, B, Cr, M, geo["taps"], geo["kw"], geo["base"], geo["rs"], geo["cs"], N, plane_in, r4(N), z.view)
        except _lib.FqssError as ex:
            assert "too short" in str(ex), str(ex)
            outcome[plane_in] = "refused"
            continue
        torch.cuda.synchronize()
        ref = flat_conv_ref(xp.double(), Wm, geo["taps"], sh, N, None if bias is None else bias.double())
        e, em = errs(z.view[:, :, :N], ref)
        outcome[plane_in] = (e, em)
        assert z.guards_intact()
        assert e <= TOL["x3s"] and em <= ELEM, (plane_in, p_min, e, em, "the last column group read shifted columns")
    print(f"{entry}, N = {N}: plane {p_old} -> {outcome[p_old]}, {p_min - 4} -> {outcome[p_min - 4]}, {p_min} -> {outcome[p_min]}")
    assert outcome[p_min - 4] == "refused" and outcome[p_min] != "refused"


# ----------------------------------------------------------------------------------------------------------------------------- layer paths
LAYER_TOL = 1e-6     # output / data gradient of a layer: both weight kinds (the kernel-level tests above hold each form to its own bound)
LAYER_CASES = {
    "halo: decoder.0 rewrite Conv2d(384, 768, 3, 1, 1) on 8 x 431": "halo",
    "phase: encoder.2 Conv2d(96, 192, (8, 1), (4, 1), (2, 0)) on 128 x 431": "phase",
}


def _layer_errs(name, got, ref, base, K):
    """base: the normwise bound at K <= 768 (the reduction length of the GEMM that made `got`), scaled as tol()"""
    e, em = errs(got, ref)
    bound = base * math.sqrt(max(1.0, K / 768))
    print(f"  {name}: {e:.2e} (elementwise {em:.2e}; bound {bound:.1e})")
    assert e <= bound and em <= elem(K), (name, e, bound, em)


@pytest.mark.parametrize("weights", ["float", "int8 codes"])
@pytest.mark.parametrize("case", list(LAYER_CASES))
def test_conv_layer_paths_against_fp64_autograd(case, weights, monkeypatch):
    """QL.conv_frames on its implicit forms (ops_dp.ConvHalo / ConvPhase) at the shipped cfg-5 widths: output, input, weight and bias
    gradients against float64 F.conv2d autograd on the same fp32 values (the existing layer tests compare the gradients only with the
    frame path); then the arena route of a table-quantized weight (`_fqss_gwq`) against the same float64 weight gradient.  Measured
    (float / int8 codes): rewrite output 9.2e-7 / 5.7e-7, input gradient 1.35e-6 / 8.3e-7, weight gradient 4.9e-7, bias 9.4e-8;
    encoder.2 output 4.2e-7 / 2.7e-7, input gradient 3.0e-7 / 1.9e-7, weight gradient 3.4e-7, bias 9.6e-8"""
    from torch import nn
    from fqss_amd import ops
    from fqss_amd.quantization.qat import qat_layers as QL
    torch.manual_seed(29)
    if LAYER_CASES[case] == "halo":
        conv, x = nn.Conv2d(384, 768, 3, 1, 1), rnd(1, 384, 8, 431, seed=31)
        expect = "fqss_conv2_fwd_wq" if weights != "float" else "fqss_conv2_fwd_x3s"
    else:
        conv, x = nn.Conv2d(96, 192, (8, 1), (4, 1), (2, 0)), rnd(1, 96, 128, 431, seed=32)
        expect = "fqss_phase_pack"
    conv = conv.to(DEV)
    Co = conv.out_channels
    w, wc = conv.weight.detach().clone(), None
    if weights == "int8 codes":
        ones = torch.ones(Co, 1, 1, device=DEV) * float(w.abs().max())
        wc = K.wq_codes(w.reshape(Co, -1, 1).contiguous(), -ones, ones)
        w = (wc.dw[:, None] * wc.idx.to(torch.float32)).view_as(conv.weight).contiguous()
    seen, real_call = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (seen.append(name), real_call(name, *a))[1])
    wq = w.clone().requires_grad_(True)
    if wc is not None:
        wq._fqss_wcodes_dgrad = wc
    conv.bias.grad = None
    xin = x.to(DEV).requires_grad_(True)
    y = ops.real(QL.conv_frames(conv, xin, wq))
    gy = rnd(*y.shape, seed=33).to(DEV)
    (y * gy).sum().backward()
    torch.cuda.synchronize()
    assert expect in seen and "fqss_frames_gather" not in seen, set(seen)
    x64, w64 = x.double().requires_grad_(True), w.cpu().double().requires_grad_(True)
    b64 = conv.bias.detach().cpu().double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, b64, conv.stride, conv.padding)
    (y64 * gy.cpu().double()).sum().backward()
    print(f"{case} / {weights}:")
    taps = conv.kernel_size[0] * conv.kernel_size[1]
    Kf, Kd = conv.in_channels * taps, Co * taps
    _layer_errs("output", y.detach().cpu(), y64.detach(), LAYER_TOL, Kf)
    _layer_errs("input gradient", xin.grad.cpu(), x64.grad, LAYER_TOL, Kd)
    _layer_errs("weight gradient", wq.grad.cpu(), w64.grad, TOL["wgrad"], 1)
    _layer_errs("bias gradient", conv.bias.grad.cpu(), b64.grad, TOL["wgrad"], 1)
    wa = w.clone()
    wa._fqss_gwq = torch.zeros_like(w)
    if wc is not None:
        wa._fqss_wcodes_dgrad = wc
    y = ops.real(QL.conv_frames(conv, x.to(DEV).requires_grad_(True), wa))
    (y * gy).sum().backward()
    torch.cuda.synchronize()
    _layer_errs("weight gradient, arena", wa._fqss_gwq.cpu(), w64.grad, TOL["wgrad"], 1)


def test_transposed_conv_layer_path_against_fp64_autograd(monkeypatch):
    """QL.convtr_frames on ops_dp.ConvTrPhase at the shipped decoder.1 shape (ConvTranspose2d(192, 96, (8, 1), (4, 1)) on 32 x 431, the
    rows 2 .. -2 the decoder keeps): output, input / weight / bias gradients against float64 conv_transpose2d autograd, and the arena
    route of a table-quantized weight.  Measured: output 3.0e-7, input gradient 4.2e-7, weight gradient 3.4e-7, bias 1.2e-7"""
    from torch import nn
    from fqss_amd import ops
    from fqss_amd.quantization.qat import qat_layers as QL
    torch.manual_seed(37)
    conv = nn.ConvTranspose2d(192, 96, (8, 1), (4, 1)).to(DEV)
    x = rnd(1, 192, 32, 431, seed=38)
    window = (-2, 2, (32 - 1) * 4 + 8 - 4)
    seen, real_call = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (seen.append(name), real_call(name, *a))[1])
    xin = x.to(DEV).requires_grad_(True)
    y = ops.real(QL.convtr_frames(conv, xin, conv.weight, window=window))
    gy = rnd(*y.shape, seed=39).to(DEV)
    (y * gy).sum().backward()
    torch.cuda.synchronize()
    assert "fqss_phase_unpack" in seen and "fqss_frames_ola" not in seen, set(seen)
    x64 = x.double().requires_grad_(True)
    w64 = conv.weight.detach().cpu().double().requires_grad_(True)
    b64 = conv.bias.detach().cpu().double().requires_grad_(True)
    y64 = F.conv_transpose2d(x64, w64, b64, conv.stride).narrow(*window)
    (y64 * gy.cpu().double()).sum().backward()
    print("decoder.1 conv_tr:")
    _layer_errs("output", y.detach().cpu(), y64.detach(), LAYER_TOL, 192 * 2)
    _layer_errs("input gradient", xin.grad.cpu(), x64.grad, LAYER_TOL, 96 * 8)
    _layer_errs("weight gradient", conv.weight.grad.cpu(), w64.grad, TOL["wgrad"], 1)
    _layer_errs("bias gradient", conv.bias.grad.cpu(), b64.grad, TOL["wgrad"], 1)
    wa = conv.weight.detach().clone()
    wa._fqss_gwq = torch.zeros_like(wa)
    y = ops.real(QL.convtr_frames(conv, x.to(DEV).requires_grad_(True), wa, window=window))
    (y * gy).sum().backward()
    torch.cuda.synchronize()
    _layer_errs("weight gradient, arena", wa._fqss_gwq.cpu(), w64.grad, TOL["wgrad"], 1)


# ----------------------------------------------------------------------------------------------------------------------------- deterministic mode
@pytest.fixture
def det_off():
    yield
    K.DetMode.off()          # (the control block is device-wide: no later test may run under it)


@pytest.mark.parametrize("scale", [1e-9, 1.0, 1e4])
def test_deterministic_sums_against_fp64(scale, det_off):
    """FQSS_DETERMINISTIC=1 arithmetic (fqss_dev.h grad_add: every split add as a two-word fixed-point integer sum on the arena's
    shadow, fqss_det_finish rounds once): the split-K weight gradient of fqss_conv2_bwd_w into a DetMode.temp_like slice of the slot-2
    pool, and the bias sums of fqss_chan_sum into a slice of the slot-0 arena.  Two runs bit-identical, and both within the float64
    bounds of the fp32-atomic path, which is measured beside them.  Operands scaled by 1e-9 (sums of a few 2^-30: the low word carries
    them) and 1e4 (the high word).  Measured at every scale: weight gradient 1.3e-7 deterministic / 1.5e-7 atomic, bias sums
    1.0e-7 .. 1.2e-7 either way."""
    plan = K.HaloPlan(13, 37, K.ConvGeom((3, 3), (1, 1), (1, 1)))
    B, Ci, Co, taps, Wp = 2, 32, 48, plan.taps, plan.Wp
    gzp = (rnd(B, Co, plan.plane_g, seed=41) * scale).to(DEV)
    xp = rnd(B, Ci, plan.plane_x, seed=42).to(DEV)
    off = plan.phg * Wp + plan.pwg
    ref_w = wgrad_ref(gzp.double(), xp.double(), taps, 3, Wp, 1, off)
    g = K.empty_act((B, Co, 1333), DEV)
    g.copy_(rnd(B, Co, 1333, seed=43) * scale)
    ref_b = g.double().sum(dim=(0, 2))
    gw_atomic, gb_atomic = torch.zeros(Co, Ci * taps, device=DEV), torch.zeros(Co, device=DEV)
    K.conv2_bwd_w(gzp, xp, gw_atomic, plan)
    K.chan_sum(g, gb_atomic)
    torch.cuda.synchronize()
    det = K.DetMode()
    arena = torch.zeros(Co * Ci * taps + 4 * Co, device=DEV)
    det.attach(0, arena)                 # (also sizes the slot-2 pool)
    det.activate()
    runs = []
    for _ in range(2):
        det.begin_backward()
        t = det.temp_like(gw_atomic)
        assert t is not None
        K.conv2_bwd_w(gzp, xp, t, plan)
        det.finish_temp(t)
        arena.zero_()
        gb = arena[Co:2 * Co]
        K.chan_sum(g, gb)
        det.finish(0)
        torch.cuda.synchronize()
        runs.append((t.clone(), gb.clone()))
    K.DetMode.off()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "deterministic mode: two runs differ"
    for what, got, ref in (("weight gradient, fp32 atomics", gw_atomic, ref_w), ("bias sums, fp32 atomics", gb_atomic, ref_b),
                           ("weight gradient, deterministic", runs[0][0], ref_w), ("bias sums, deterministic", runs[0][1], ref_b)):
        e, em = errs(got, ref)
        print(f"scale {scale:g}, {what}: {e:.2e} (elementwise {em:.2e})")
        assert e <= TOL["wgrad"] and em <= ELEM, (what, e, em)


# ----------------------------------------------------------------------------------------------------------------------------- frozen weights
def test_frozen_regrouped_weight_follows_every_write():
    """ops_dp._frozen_cache keeps the phase-regrouped image of a frozen (requires_grad=False) weight on the parameter; it must follow
    every write to that weight: an in-place copy_ under no_grad, `weight.data = new` (a new tensor: the version counter stays) and a
    raw-pointer write through the library (K.axpby_).  After each, the no_grad forward equals float64 F.conv1d of the new weight."""
    from torch import nn
    from fqss_amd import ops
    from fqss_amd.quantization.qat import qat_layers as QL
    torch.manual_seed(43)
    conv = nn.Conv1d(16, 32, 8, 4, 2).to(DEV).requires_grad_(False)
    x = rnd(2, 16, 1336, seed=44).to(DEV)

    def check(what):
        with torch.no_grad():
            y = ops.real(QL.conv_frames(conv, x, conv.weight))
        torch.cuda.synchronize()
        ref = F.conv1d(x.double(), conv.weight.double(), conv.bias.double(), 4, 2)
        e, em = errs(y, ref)
        print(f"{what}: {e:.2e} (elementwise {em:.2e})")
        assert e <= TOL["x3s"] and em <= ELEM, (what, e, em)

    check("first forward")
    assert getattr(conv.weight, "_fqss_regroup", None) is not None, "the forward did not go through the frozen cache"
    with torch.no_grad():
        conv.weight.copy_(rnd(32, 16, 8, seed=45, scale=0.25).to(DEV))
    check("after copy_")
    conv.weight.data = rnd(32, 16, 8, seed=46, scale=0.25).to(DEV)
    check("after weight.data = new")
    K.axpby_(conv.weight.view(32, -1), rnd(32, 16 * 8, seed=47).to(DEV), 0.5)
    check("after K.axpby_ into the weight")
