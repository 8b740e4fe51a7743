"""The sequence kernels of the dual-path models at kernel level against float64: the LDS-resident attention core (csrc/attn.hip:
fqss_attn_fwd / fqss_attn_bwd, every template instance of k_attn_fwd, k_attn_fwd_mfma, k_attn_bwd, k_attn_bwd_mfma and both branches
of fill_head) and the LSTM recurrence (csrc/lstm.hip: fqss_lstm_fwd, fqss_lstm_bwd, fqss_lstm_bwd_b, fqss_lstm_bwd_b4; the register-
resident H = 128 kernels and the generic ones).  The C entry points are called through fqss_amd._lib with explicit leading dimensions,
so no Python dispatcher can reroute a case (kernels.attn_fwd sends aligned head_dim-16 / 32 views to csrc/attn_long.hip).

Contract under test (include/fqss.h).  Attention: rows [l*B + b], head h = columns [h*hd, (h+1)*hd), every operand and output with
its own leading dimension; stats [B*nh][L][2] = (row maximum of the logits, row sum of exp(s - max)), written by every forward form
and readable by every backward form, csrc/attn_long.hip included.  LSTM: pre [S][B][2][4H] (gate order i, f, g, o), whh [2][4H][H],
bhh [2][4H], zero initial state, the reverse direction walks t = S-1 .. 0; gsav = the four gate activations, csav = c | tanh(c) per
direction; the bias sums are ADDED into their buffers.  Operands sit in NaN-filled buffers (a read outside a head's block poisons the
result), outputs are blocks of NaN-filled buffers (a write outside shows up, a skipped element keeps its NaN).

References: plain float64 torch on the CPU with autograd (attn_ref, lstm_ref below).  Error measure per tensor:
e_norm = ||got - ref64|| / ||ref64|| and e_elem = max |got - ref64| / rms(ref64); where ref64 is zero (dq, dk at L = 1; dq with all
keys equal) max |got| is bounded by the same constant times the scale of the terms that cancel (rms(go) rms(v) rms(k) for dq).  The
yardstick is the same formula in torch fp32 on the CPU, printed beside every kernel figure.

Measured on the MI355X, largest e_elem / e_norm over all cases of a family, beside torch fp32 on the CPU on the same cases (every
maximum but the VALU-family gradients of the random cases comes from the "logits ~30" cases, where fp32 itself is that far off):
  attention, VALU kernels (k_attn_fwd, k_attn_bwd)       kernel                fp32
    o                                                    9.3e-6 / 6.4e-7       9.0e-6 / 6.3e-7
    row maximum, row sum                                 4.2e-7, 7.8e-6        4.2e-7, 7.4e-6       (e_norm 1.8e-7, 1.0e-6)
    dq, dk, dv                                           1.3e-5, 2.4e-5, 4.6e-6   1.3e-5, 2.4e-5, 4.4e-6   (e_norm <= 1.4e-6)
  attention, MFMA kernels (k_attn_fwd_mfma, k_attn_bwd_mfma)
    o                                                    1.0e-5 / 8.0e-7       1.0e-5 / 8.0e-7
    row maximum, row sum                                 4.8e-7, 8.0e-6        4.8e-7, 8.0e-6       (e_norm 1.1e-7, 1.2e-6)
    dq, dk, dv                                           2.9e-5, 2.4e-5, 9.6e-6   2.9e-5, 2.4e-5, 9.6e-6   (e_norm <= 2.0e-6)
    without the "logits ~30" cases every figure of both families is <= 5.7e-6 / 6.1e-7 (fp32: <= 7.1e-6 / 4.3e-7)
    zero reference (dq with all keys equal), relative to rms(go) rms(v) rms(k): 4.0e-7 VALU, 1.4e-6 MFMA (fp32 2.3e-7, 7.4e-7); L = 1: 0
  pairings with csrc/attn_long.hip at L = 250: o 2.8e-6 / 2.9e-7, log-sum-exp 8.5e-8 / 2.1e-8, dq, dk, dv <= 4.5e-6 / 3.7e-7
  LSTM, H = 128 (k_lstm_fwd_st<128>, k_lstm_bwd<128>)    kernel                fp32
    hout, gsav, csav                                     9.3e-7, 2.5e-7, 1.0e-6   7.6e-7, 4.9e-7, 1.0e-6   (e_norm <= 1.0e-7)
    dG                                                   1.1e-5 / 2.5e-7       8.2e-6 / 2.1e-7      (saturated gates; else <= 4.1e-6)
    bias sums (fp32 atomics and deterministic mode)      3.7e-6 / 4.4e-7       1.2e-6 / 2.1e-7
  LSTM, generic kernels (k_lstm_fwd, k_lstm_bwd<0>), H = 1 .. 256
    hout, gsav, csav                                     8.4e-7, 5.1e-7, 7.4e-7   7.7e-7, 3.6e-7, 7.6e-7   (e_norm <= 9.5e-8)
    dG                                                   5.3e-6 / 2.2e-7       5.7e-6 / 2.1e-7
    bias sums                                            1.9e-6 / 3.2e-7       1.3e-6 / 2.3e-7
The kernels are as exact as torch's fp32 on every tensor.  The bounds (ATTN_BOUND, LSTM_BOUND) are one constant per family and tensor,
at most 4 x the largest value above (the kernels are deterministic: the factor covers other seeds); they do not grow with L or S B,
no such growth was seen beyond what the constants cover.  Each bound is asserted to stay 10 x below what a wrong kernel gives, computed per
case in float64 on the CPU.  Attention with the last key dropped: e_elem >= 0.18 on o and dq, >= 1.3 on dk and dv; with q rounded to
bf16: >= 3.8e-3 on every tensor (smallest: dq at L = 9, head_dim 4).  The LSTM with whh rounded to bf16: hout >= 1.6e-4, d pre >= 5.8e-4
(smallest: H = 4 at S = 2; H = 1 and 3 at S = 5: 4.4e-4 / 1.5e-3 -- a handful of weights and steps), >= 1.0e-3 / 1.8e-3 in every case
with H >= 12; the largest hout bound, 3.5e-6, is 45 x below the smallest.  The floors are not taken where the mutation is
void by construction: L = 1; q -> bf16 when all keys are equal (the softmax stays uniform); the LSTM at S = 1 (h_0 = 0: whh is never
used) and with gates saturated on purpose.

H below 4 (the entry check admits any H > 0): the generic kernels launch cdiv(4H, 64) * 64 >= 64 threads, gate rows j < 4H and cell
threads tid < 2H are guarded, W_hh rows are clamped to row 0 for idle threads, and the LDS images are sized by H (hs: 2 (H + 16), gs:
8H, ps: 8H floats): every index stays inside its array at H = 1 and H = 3, which run below like any other size."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
K = None
_lib = None
DEV = "cuda"
NAN = float("nan")
EINVAL = -22
LDS_BYTES = 160 * 1024                   # ensure_lds of csrc/attn.hip
# per kernel family and tensor: (e_elem bound, e_norm bound)
ATTN_BOUND = {
    "valu": {"o": (3e-5, 2.5e-6), "max": (1.5e-6, 6e-7), "sum": (3e-5, 4e-6), "gq": (5e-5, 5e-6), "gk": (9e-5, 5e-6), "gv": (1.6e-5, 1.6e-6)},
    "mfma": {"o": (3.5e-5, 3e-6), "max": (1.5e-6, 4e-7), "sum": (3e-5, 4e-6), "gq": (1e-4, 7e-6), "gk": (9e-5, 7e-6), "gv": (3.5e-5, 3e-6)},
    # csrc/attn_long.hip (the cross pairing only, operands of scale 0.8); lse = m + log(l), see test_attention_stats_pair_across_families
    "long": {"o": (1e-5, 1e-6), "lse": (3e-7, 8e-8), "gq": (1.4e-5, 1.4e-6), "gk": (1.6e-5, 1.4e-6), "gv": (1.5e-5, 1.4e-6)},
}
LSTM_BOUND = {
    "st128": {"hout": (3.5e-6, 4e-7), "gsav": (1e-6, 1.6e-7), "csav": (4e-6, 3.2e-7), "dG": (4e-5, 1e-6), "bias": (1.4e-5, 1.6e-6)},
    "generic": {"hout": (3e-6, 3.5e-7), "gsav": (2e-6, 1.6e-7), "csav": (2.8e-6, 3e-7), "dG": (2e-5, 8e-7), "bias": (7e-6, 1.2e-6)},
}
LAZY_MAX = 8.0                           # csrc/attn_long.hip kLazy: how far the streaming forward's reference value may lag the row maximum


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


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def errs(a, ref):
    """(max |a - ref| / rms(ref), ||a - ref|| / ||ref||) of a against a float64 reference"""
    d = a.double().cpu() - ref
    return float(d.abs().max() / rms(ref)), float(d.norm() / ref.norm())


def stream():
    return torch.cuda.current_stream().cuda_stream


def rc_of(name, *args):
    """status of an entry point, without the exception _lib.call makes of it"""
    return _lib._bind(name)(*args)


def refused(name, *args):
    """the entry returns FQSS_EINVAL and fqss_last_error names it"""
    rc = rc_of(name, *args)
    msg = _lib.load().fqss_last_error().decode()
    torch.cuda.synchronize()
    assert rc == EINVAL and name in msg, (name, rc, msg)
    return msg


class Block:
    """[rows][E] floats with row stride ld, `off` floats into a NaN-filled flat device buffer that begins and ends with G guard floats
    (the buffer is 256-B aligned: the block's base is 16-B aligned iff off % 4 == 0)"""
    G = 64

    def __init__(self, rows, E, ld, off=0, fill=None):
        assert ld >= E
        self.rows, self.E, self.ld, self.off = rows, E, ld, self.G + off
        self.buf = torch.full((self.off + rows * ld + self.G,), NAN, device=DEV)
        assert self.buf.data_ptr() % 256 == 0
        self.view = self.buf.as_strided((rows, E), (ld, 1), self.off)
        if fill is not None:
            self.view.copy_(fill.reshape(rows, E))
        self.ptr = self.buf.data_ptr() + 4 * self.off

    def written_inside_only(self):
        """every element of the block finite, every other float of the buffer still NaN"""
        inside = torch.zeros_like(self.buf, dtype=torch.bool)
        inside.as_strided((self.rows, self.E), (self.ld, 1), self.off).fill_(True)
        return bool(torch.isfinite(self.buf[inside]).all()) and bool(torch.isnan(self.buf[~inside]).all())

    def untouched(self):
        return bool(torch.isnan(self.buf).all())

    def cpu(self, *shape):
        return self.view.cpu().reshape(*shape)


def same_bits(a, b):
    return a.shape == b.shape and not bool(torch.isnan(a).any()) and bool(torch.equal(a, b))


# ============================================================================================================================ attention
def attn_ref(q, k, v, go, nh, dtype=torch.float64, drop_last=False, q_bf16=False):
    """softmax(q k^T) v per (sequence, head) of [L, B, E] operands in `dtype`, and autograd's gradients for the output gradient go
    -> dict of o, gq, gk, gv [L, B, E], max / sum [B*nh, L] (row maximum, row sum of exp(s - max)), s / p (logits, probabilities).
    drop_last / q_bf16: the two wrong kernels of the margin check (the last key ignored; q rounded to bf16)"""
    L, B, E = q.shape
    hd = E // nh
    if q_bf16:
        q = q.bfloat16().float()
    q, k, v = (t.to(dtype).clone().requires_grad_(True) for t in (q, k, v))
    heads = lambda t: t.reshape(t.shape[0], B * nh, hd).permute(1, 0, 2)      # noqa: E731
    Lk = L - 1 if drop_last else L
    s = heads(q) @ heads(k[:Lk]).transpose(1, 2)
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    den = e.sum(-1, keepdim=True)
    p = e / den
    o = (p @ heads(v[:Lk])).permute(1, 0, 2).reshape(L, B, E)
    o.backward(go.to(dtype))
    return {"o": o.detach(), "gq": q.grad, "gk": k.grad, "gv": v.grad, "max": m.detach()[..., 0], "sum": den.detach()[..., 0],
            "lse": (m + den.log()).detach()[..., 0], "s": s.detach(), "p": p.detach()}


def attn_operands(L, B, nh, hd, kind, seed):
    """q (already divided by sqrt(hd), as the layer hands it over), k, v, go: [L, B, E] fp32 on the CPU.  kind: "random" (0.8-scaled, as
    the layer tests), "large" (logits of magnitude ~30: exp(s - max) underflows for most keys), "uniform" (all keys of a head equal:
    p = 1 / L), "pos" / "neg" (every logit positive / negative: a padding key's logit 0 would be the minimum / maximum)"""
    E = nh * hd
    X = rnd(L, B, 3 * E, seed=seed, scale=0.8)
    q, k, v = X[..., :E] / math.sqrt(hd), X[..., E:2 * E].clone(), X[..., 2 * E:].clone()
    if kind == "large":
        q, k = q * (12.5 / 0.8), k / 0.8                       # logits ~ N(0, 10^2): the row maximum is near 30
    elif kind == "uniform":
        k = k[:1].expand(L, B, E).clone()
    elif kind in ("pos", "neg"):
        q, k = q.abs() + 0.05, (k.abs() + 0.05) * (1.0 if kind == "pos" else -1.0)
    else:
        assert kind == "random"
    return q.contiguous(), k, v, rnd(L, B, E, seed=seed + 1)


# operand placement -> (ld, [float offsets of q, k, v, go])
PLACE = {
    "wide": lambda E: (3 * E, [0, E, 2 * E, E]),               # column blocks of a wide buffer: 16-B aligned rows (E % 4 == 0)
    "ld%4": lambda E: (3 * E + 1 + (3 * E) % 2, [0, E, 2 * E, E]),    # ld % 4 != 0 (E % 4 == 0: ld = 3E + 1)
    "base+1": lambda E: (3 * E, [1, E + 1, 2 * E + 1, E + 1]),  # base pointer one float past a 16-B boundary
}


def fwd_family(L, hd):
    return "mfma" if hd == 32 and L <= 256 else "valu"


def bwd_family(L, hd):
    return "mfma" if hd in (16, 32) and L <= 256 else "valu"


def fwd_lds(L, hd):
    if fwd_family(L, hd) == "mfma":
        return 3 * ((L + 31) // 32 * 32) * (hd + 1) * 4
    return 2 * L * hd * 4


def bwd_lds(L, hd):
    if bwd_family(L, hd) == "mfma":
        Lp = (L + 31) // 32 * 32
        return (4 * Lp * (hd + 1) + 3 * Lp) * 4
    return (4 * L * hd + 3 * L) * 4


class AttnRun:
    """one forward (and optionally backward) of the LDS-resident kernels on CPU operands, every tensor in a Block of its own"""

    def __init__(self, q, k, v, go, nh, place="wide", observe=False):
        L, B, E = q.shape
        self.L, self.B, self.nh, self.hd, self.E = L, B, nh, E // nh, E
        ld, offs = PLACE[place](E)
        R = L * B
        self.q, self.k, self.v, self.go = (Block(R, E, ld, o, t) for o, t in zip(offs, (q, k, v, go)))
        self.o = Block(R, E, 2 * E, E)
        self.stats = torch.full((B * nh, L, 2), NAN, device=DEV)
        self.ws = torch.tensor([-1, 0, -1, 0], dtype=torch.int32, device=DEV) if observe else None
        self.gq, self.gk, self.gv = Block(R, E, 3 * E, 0), Block(R, E, 3 * E, E), Block(R, E, E + 1, 0)

    def fwd_args(self):
        ws = self.ws
        return (self.q.ptr, self.k.ptr, self.v.ptr, self.o.ptr, self.stats.data_ptr(), self.L, self.B, self.nh, self.hd, self.q.ld,
                self.k.ld, self.v.ld, self.o.ld, None if ws is None else ws.data_ptr(), None if ws is None else ws.data_ptr() + 8, stream())

    def bwd_args(self, o=None, stats=None):
        o, stats = o or self.o, self.stats if stats is None else stats
        return (self.q.ptr, self.k.ptr, self.v.ptr, o.ptr, self.go.ptr, stats.data_ptr(), self.gq.ptr, self.gk.ptr, self.gv.ptr, self.L,
                self.B, self.nh, self.hd, self.q.ld, self.k.ld, self.v.ld, o.ld, self.go.ld, self.gq.ld, self.gk.ld, self.gv.ld, stream())

    def forward(self):
        assert fwd_lds(self.L, self.hd) <= LDS_BYTES, "a launching case must stay inside the kernel's LDS limit"
        _lib.call("fqss_attn_fwd", *self.fwd_args())
        torch.cuda.synchronize()
        assert self.o.written_inside_only(), "o: a NaN inside the block or a write outside it"
        assert bool(torch.isfinite(self.stats).all()), "stats not fully written"
        return self

    def backward(self, o=None, stats=None):
        assert bwd_lds(self.L, self.hd) <= LDS_BYTES
        _lib.call("fqss_attn_bwd", *self.bwd_args(o, stats))
        torch.cuda.synchronize()
        for name in ("gq", "gk", "gv"):
            assert getattr(self, name).written_inside_only(), f"{name}: a NaN inside the block or a write outside it"
        return self

    def outputs(self, with_grads=True):
        shape = (self.L, self.B, self.E)
        out = {"o": self.o.cpu(*shape), "max": self.stats[..., 0].cpu(), "sum": self.stats[..., 1].cpu()}
        if with_grads:
            out.update({n: getattr(self, n).cpu(*shape) for n in ("gq", "gk", "gv")})
        return out

    def observed(self):
        def dec(u):
            u = int(u) & 0xffffffff
            u = (u & 0x7fffffff) if (u & 0x80000000) else (~u & 0xffffffff)
            return float(np.array([u], dtype=np.uint32).view(np.float32)[0])
        return [dec(u) for u in self.ws.cpu().tolist()]


def check_attn(tag, got, ref, ref32, family_of, ops, fails):
    """print e_elem / e_norm of every tensor in `got` beside torch fp32's, collect the bounds it misses.  A zero reference (the terms
    cancel exactly): max |got| against the bound times the scale of the cancelling terms"""
    q, k, v, go = ops
    cancel = {"gq": rms(go) * rms(v) * rms(k), "gk": rms(go) * rms(v) * rms(q)}
    for name, g in got.items():
        fam = family_of[name]
        b_elem, b_norm = ATTN_BOUND[fam][name]
        r = ref[name]
        if name in cancel and float(r.abs().max()) <= 1e-12 * cancel[name]:
            e = float(g.double().abs().max()) / cancel[name]
            e32 = float(ref32[name].double().abs().max()) / cancel[name]
            print(f"MEAS attn {fam} {name} zero-ref {e:.2e} - fp32 {e32:.2e} - | {tag}")
            if not e <= b_elem:
                fails.append((tag, name, "zero reference", e, b_elem))
            continue
        e_elem, e_norm = errs(g, r)
        f_elem, f_norm = errs(ref32[name], r)
        print(f"MEAS attn {fam} {name} e_elem {e_elem:.2e} e_norm {e_norm:.2e} fp32 {f_elem:.2e} {f_norm:.2e} | {tag}")
        if not (e_elem <= b_elem and e_norm <= b_norm):
            fails.append((tag, name, e_elem, e_norm, b_elem, b_norm))


def check_attn_floors(tag, ops, nh, ref, kind, families):
    """the bounds stay 10 x below what the two wrong kernels give on this case's operands"""
    q, k, v, go = ops
    L = q.shape[0]
    if L == 1:
        return
    muts = {"last key dropped": attn_ref(q, k, v, go, nh, drop_last=True)}
    if kind != "uniform":
        muts["q rounded to bf16"] = attn_ref(q, k, v, go, nh, q_bf16=True)
    for what, mut in muts.items():
        for name in ("o", "gq", "gk", "gv"):
            r = ref[name]
            if float(r.abs().max()) == 0.0 or (kind == "uniform" and name == "gq"):
                continue
            floor = errs(mut[name], r)[0]
            print(f"FLOOR attn {name} {what} {floor:.2e} | {tag}")
            for fam in families:
                assert ATTN_BOUND[fam][name][0] * 10 <= floor, (tag, what, name, floor, fam)


# id: "<forward kernel> / <backward kernel>, what the shape is for" -> (L, B, nh, hd, kind)
ATTN_CASES = {
    "fwd<2> / bwd<2>, L 37, several heads": (37, 4, 4, 2, "random"),
    "fwd<2> / bwd<2>, L 1, one head, B 1": (1, 1, 1, 2, "random"),
    "fwd<4> / bwd<4>, L 9": (9, 5, 4, 4, "random"),
    "fwd<4> / bwd<4>, L 300: block loop wraps": (300, 1, 3, 4, "random"),
    "fwd<8> / bwd<8>, L 31": (31, 3, 4, 8, "random"),
    "fwd<8> / bwd<8>, L 257, one head": (257, 2, 1, 8, "random"),
    "fwd<8> / bwd<8>, L 200, B 1": (200, 1, 4, 8, "random"),
    "fwd<8> / bwd<8>, L 64, all keys equal": (64, 2, 2, 8, "uniform"),
    "fwd<8> / bwd<8>, L 250, logits ~30": (250, 1, 2, 8, "large"),
    "fwd<16> / bwd_mfma<16>, L 1": (1, 2, 2, 16, "random"),
    "fwd<16> / bwd_mfma<16>, L 31": (31, 1, 1, 16, "random"),
    "fwd<16> / bwd_mfma<16>, L 32": (32, 3, 2, 16, "random"),
    "fwd<16> / bwd_mfma<16>, L 33": (33, 2, 4, 16, "random"),
    "fwd<16> / bwd_mfma<16>, L 128: grid.y 1": (128, 1, 2, 16, "random"),
    "fwd<16> / bwd_mfma<16>, L 129: grid.y 2": (129, 1, 2, 16, "random"),
    "fwd<16> / bwd_mfma<16>, L 194 (chunks)": (194, 3, 4, 16, "random"),
    "fwd<16> / bwd_mfma<16>, L 250 (chunk length)": (250, 3, 4, 16, "random"),
    "fwd<16> / bwd_mfma<16>, L 250, logits ~30": (250, 2, 2, 16, "large"),
    "fwd<16> / bwd_mfma<16>, L 255": (255, 1, 1, 16, "random"),
    "fwd<16> / bwd_mfma<16>, L 256: last MFMA length": (256, 2, 2, 16, "random"),
    "fwd<16> / bwd<16>, L 257: first VALU length": (257, 2, 2, 16, "random"),
    "fwd<16> / bwd<16>, L 300: block loop wraps": (300, 1, 4, 16, "random"),
    "fwd_mfma<32> / bwd_mfma<32>, L 1": (1, 1, 2, 32, "random"),
    "fwd_mfma<32> / bwd_mfma<32>, L 31": (31, 2, 1, 32, "random"),
    "fwd_mfma<32> / bwd_mfma<32>, L 32": (32, 1, 2, 32, "random"),
    "fwd_mfma<32> / bwd_mfma<32>, L 33": (33, 3, 2, 32, "random"),
    "fwd_mfma<32> / bwd_mfma<32>, L 128: grid.y 1": (128, 2, 1, 32, "random"),
    "fwd_mfma<32> / bwd_mfma<32>, L 129: grid.y 2": (129, 1, 2, 32, "random"),
    "fwd_mfma<32> / bwd_mfma<32>, L 200, logits ~30": (200, 1, 2, 32, "large"),
    "fwd_mfma<32> / bwd_mfma<32>, L 250 (chunk length)": (250, 3, 8, 32, "random"),
    "fwd_mfma<32> / bwd_mfma<32>, L 255": (255, 1, 1, 32, "random"),
    "fwd_mfma<32> / bwd_mfma<32>, L 256: last MFMA length": (256, 1, 2, 32, "random"),
    "fwd_mfma<32> / bwd_mfma<32>, L 256, all keys equal": (256, 1, 2, 32, "uniform"),
    "fwd<32> / bwd<32>, L 257: first VALU length": (257, 1, 2, 32, "random"),
    "fwd<32> / bwd<32>, L 300: block loop wraps": (300, 2, 2, 32, "random"),
}


@pytest.mark.parametrize("case", list(ATTN_CASES))
def test_attention_against_fp64(case):
    """fqss_attn_fwd / fqss_attn_bwd on column blocks of wide buffers (ld = 3E) against float64: o, the saved statistics (row maximum,
    row sum), dq, dk, dv within the family's bounds; every output block fully written and nothing outside it; a second call gives
    the same bits (csrc/attn.hip: "no atomics, deterministic").  The id names the kernels the shape selects; the selection rule is
    restated in fwd_family / bwd_family and checked against the id."""
    L, B, nh, hd, kind = ATTN_CASES[case]
    names = case.split(",")[0].split(" / ")
    assert names[0] == ("fwd_mfma<%d>" if fwd_family(L, hd) == "mfma" else "fwd<%d>") % hd
    assert names[1] == ("bwd_mfma<%d>" if bwd_family(L, hd) == "mfma" else "bwd<%d>") % hd
    ops = attn_operands(L, B, nh, hd, kind, seed=100 + L + hd)
    ref, ref32 = attn_ref(*ops, nh), attn_ref(*ops, nh, dtype=torch.float32)
    run = AttnRun(*ops, nh).forward().backward()
    got = run.outputs()
    again = AttnRun(*ops, nh).forward().backward().outputs()
    fam = {n: fwd_family(L, hd) for n in ("o", "max", "sum")}
    fam.update({n: bwd_family(L, hd) for n in ("gq", "gk", "gv")})
    fails = []
    check_attn(case, got, ref, ref32, fam, ops, fails)
    if kind == "uniform" and L & (L - 1) == 0:
        print(f"uniform softmax: row sums {float(got['sum'].min())} .. {float(got['sum'].max())} (exactly L = {L} expected)")
        assert bool((got["sum"] == float(L)).all()), "all keys equal: every exp(s - max) is exactly 1"
    assert not fails, fails
    for n in got:
        assert same_bits(got[n], again[n]), f"{n}: two calls on the same operands differ"
    check_attn_floors(case, ops, nh, ref, kind, set(fam.values()))


def max_len(lds_of, hd):
    L = 257                                # (head_dim 32: the VALU forms begin here)
    while lds_of(L + 1, hd) <= LDS_BYTES:
        L += 1
    return L


def test_attention_lds_limits_at_head_dim_32():
    """The largest L each VALU form admits at head_dim 32 by the 160-KiB rule of ensure_lds (forward: K, V = 2 L hd floats -> 640;
    backward: q, k, v, dO and three row vectors = (4 L hd + 3 L) floats -> 312) runs and meets the bounds; one past it is refused
    with FQSS_EINVAL, a message that names the entry, and no write (NaN-filled outputs stay NaN).  A forward can succeed where its
    backward refuses (312 < L <= 640): the refusal is clean."""
    hd, nh, B = 32, 1, 1
    Lf, Lb = max_len(fwd_lds, hd), max_len(bwd_lds, hd)
    assert (Lf, Lb) == (640, 312)
    fails = []
    fam = {n: "valu" for n in ("o", "max", "sum", "gq", "gk", "gv")}
    ops = attn_operands(Lb, B, nh, hd, "random", seed=7)
    got = AttnRun(*ops, nh).forward().backward().outputs()
    check_attn(f"fwd<32> / bwd<32>, L {Lb}: largest backward", got, attn_ref(*ops, nh), attn_ref(*ops, nh, dtype=torch.float32), fam, ops, fails)
    ops = attn_operands(Lf, B, nh, hd, "random", seed=8)
    run = AttnRun(*ops, nh).forward()
    ref = attn_ref(*ops, nh)
    check_attn(f"fwd<32>, L {Lf}: largest forward", run.outputs(False), ref, attn_ref(*ops, nh, dtype=torch.float32), fam, ops, fails)
    assert not fails, fails
    # ... whose backward is refused: nothing launched, nothing written
    msg = refused("fqss_attn_bwd", *run.bwd_args())
    assert "LDS" in msg and run.gq.untouched() and run.gk.untouched() and run.gv.untouched()
    ops = attn_operands(Lb + 1, B, nh, hd, "random", seed=9)
    run = AttnRun(*ops, nh).forward()
    refused("fqss_attn_bwd", *run.bwd_args())
    assert run.gq.untouched() and run.gk.untouched() and run.gv.untouched()
    ops = attn_operands(Lf + 1, B, nh, hd, "random", seed=10)
    run = AttnRun(*ops, nh)
    msg = refused("fqss_attn_fwd", *run.fwd_args())
    assert "LDS" in msg and run.o.untouched() and bool(torch.isnan(run.stats).all())


PLACE_CASES = {
    "fill_head scalar against float4, fwd_mfma<32> / bwd_mfma<32>, L 250": (250, 2, 2, 32),
    "fill_head scalar against float4, fwd_mfma<32> / bwd_mfma<32>, L 33, B 1": (33, 1, 3, 32),
    "fill_head scalar against float4, fwd<16> / bwd_mfma<16>, L 250": (250, 3, 4, 16),
    "fill_head scalar against float4, fwd<16> / bwd_mfma<16>, L 129": (129, 1, 1, 16),
    "fwd<8> / bwd<8>, L 40": (40, 2, 4, 8),
    "fwd<32> / bwd<32>, L 257": (257, 1, 2, 32),
}


@pytest.mark.parametrize("case", list(PLACE_CASES))
def test_attention_operand_placement_is_bit_identical(case):
    """The same values as column blocks of a 16-B aligned wide buffer, with ld % 4 != 0, and with the base pointer one float off
    alignment: the last two send fill_head (the MFMA kernels' LDS fill) through its scalar branch.  Only the loads differ, so o,
    stats and the gradients are bit-identical across the three; the VALU kernels, which load scalars anyway, likewise."""
    L, B, nh, hd = PLACE_CASES[case]
    ops = attn_operands(L, B, nh, hd, "random", seed=31 + L)
    outs = {}
    for place in PLACE:
        run = AttnRun(*ops, nh, place)
        aligned = run.q.ptr % 16 == 0 and run.q.ld % 4 == 0
        assert aligned == (place == "wide") and (run.k.ptr % 16 == 0) == (place != "base+1")
        outs[place] = run.forward().backward().outputs()
    ref = attn_ref(*ops, nh)
    print(f"{case}: o e_elem {errs(outs['ld%4']['o'], ref['o'])[0]:.2e} on the scalar fill")
    for place in ("ld%4", "base+1"):
        for n, t in outs["wide"].items():
            assert same_bits(t, outs[place][n]), f"{n}: placement {place!r} differs from the aligned wide buffer"


def test_attention_refuses_bad_arguments():
    """argument checks of both entries: a lone observer, a head_dim that is not built, a row stride below the embedding width, L = 0:
    FQSS_EINVAL, a message naming the entry, outputs untouched"""
    ops = attn_operands(8, 2, 2, 8, "random", seed=3)
    run = AttnRun(*ops, 2, observe=True)
    a = list(run.fwd_args())
    for bad in ({13: None}, {14: None}, {8: 3}, {8: 64}, {9: 15}, {12: 15}, {5: 0}, {6: 0}, {7: 0}):
        b = list(a)
        for i, val in bad.items():
            b[i] = val
        refused("fqss_attn_fwd", *b)
    assert run.o.untouched() and bool(torch.isnan(run.stats).all())
    run.ws = None
    run.forward()
    a = list(run.bwd_args())
    for bad in ({12: 3}, {12: 64}, {13: 15}, {18: 15}, {20: 15}, {9: 0}, {10: 0}, {6: None}):
        b = list(a)
        for i, val in bad.items():
            b[i] = val
        refused("fqss_attn_bwd", *b)
    assert run.gq.untouched() and run.gk.untouched() and run.gv.untouched()


OBS_CASES = {
    "fwd<16> (VALU), L 250, every logit positive": (250, 2, 2, 16, "pos"),
    "fwd<16> (VALU), L 70, every logit negative": (70, 3, 2, 16, "neg"),
    "fwd<8> (VALU), L 300, random": (300, 1, 2, 8, "random"),
    "fwd_mfma<32>, L 250 (padding keys 250 .. 255), every logit positive": (250, 2, 2, 32, "pos"),
    "fwd_mfma<32>, L 33 (padding keys 33 .. 63), every logit negative": (33, 2, 1, 32, "neg"),
    "fwd_mfma<32>, L 129, grid.y 2, random": (129, 1, 2, 32, "random"),
}


@pytest.mark.parametrize("case", list(OBS_CASES))
def test_attention_observers(case):
    """obs_attn / obs_soft: the decoded (min, max) of the logits and of the probabilities against float64, at the tolerances of
    test_gpu_dptnet.py::test_attention_kernels (logits: rtol 1e-5, atol 1e-6; probabilities: rtol 1e-4).  With every logit positive
    (negative) the logit 0 of an MFMA padding key would be the minimum (maximum) if it entered.  Without observers the output is
    bit-identical to the observed run."""
    L, B, nh, hd, kind = OBS_CASES[case]
    ops = attn_operands(L, B, nh, hd, kind, seed=57 + L)
    ref = attn_ref(*ops, nh)
    if kind != "random":
        assert float(ref["s"].min()) > 0 if kind == "pos" else float(ref["s"].max()) < 0
    run = AttnRun(*ops, nh, observe=True).forward()
    smin, smax, pmin, pmax = run.observed()
    print(f"{case}: logits [{smin:.7g}, {smax:.7g}] float64 [{float(ref['s'].min()):.7g}, {float(ref['s'].max()):.7g}]; "
          f"probabilities [{pmin:.7g}, {pmax:.7g}] float64 [{float(ref['p'].min()):.7g}, {float(ref['p'].max()):.7g}]")
    np.testing.assert_allclose([smin, smax], [float(ref["s"].min()), float(ref["s"].max())], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose([pmin, pmax], [float(ref["p"].min()), float(ref["p"].max())], rtol=1e-4, atol=1e-12)
    plain = AttnRun(*ops, nh).forward().outputs(False)
    for n, t in run.outputs(False).items():
        assert same_bits(t, plain[n]), f"{n}: the observed run differs from the plain one"


@pytest.mark.parametrize("hd", [16, 32])
def test_attention_stats_pair_across_families(hd):
    """stats written by either forward family (fqss_attn_fwd here; fqss_attn_long_fwd of csrc/attn_long.hip through K.attn_long_fwd) are
    read by either backward family: all four pairings at L = 250 meet the gradient bounds (of the less exact family of a pair).
    kernels.attn_bwd relies on this whenever go is not a 3-D view.  What the two families share is (m, l) with l = sum_j exp(s_j - m),
    of which every backward uses exp(s - m) / l alone.  fqss_attn_fwd saves the row maximum itself as m (checked against float64 in
    test_attention_against_fp64 and here); the streaming forward moves its reference value lazily, so its m is only known to lie in
    [max - 8, max] (measured here: max and sum as such are off by e_norm 0.3 / 0.7) and the invariant m + log(l) = the row's
    log-sum-exp is what meets float64."""
    L, B, nh = 250, 2, 4
    E = nh * hd
    ops = attn_operands(L, B, nh, hd, "random", seed=77 + hd)
    ref, ref32 = attn_ref(*ops, nh), attn_ref(*ops, nh, dtype=torch.float32)
    fails = []
    run = AttnRun(*ops, nh).forward()
    qd, kd, vd, god = (t.to(DEV) for t in ops)
    o_long, st_long = K.attn_long_fwd(qd, kd, vd, nh, False)
    torch.cuda.synchronize()
    fwd = {"lds": (run.o, run.stats, fwd_family(L, hd)), "long": (Block(L * B, E, E, 0, o_long), st_long, "long")}
    for fname, (o, st, ffam) in fwd.items():
        m, l = st[..., 0].cpu(), st[..., 1].cpu()
        if fname == "lds":
            got = {"o": o.cpu(L, B, E), "max": m, "sum": l}
        else:
            got = {"o": o.cpu(L, B, E), "lse": m.double() + l.double().log()}
            lag = ref["max"] - m.double()
            print(f"head_dim {hd}, forward long: row maximum - m in [{float(lag.min()):.3g}, {float(lag.max()):.3g}]")
            assert float(lag.min()) >= -1e-5 and float(lag.max()) <= LAZY_MAX + 1e-5
        check_attn(f"head_dim {hd}, forward {fname}", got, ref, ref32, {n: ffam for n in got}, ops, fails)
        for bname in ("lds", "long"):
            if bname == "lds":
                r = AttnRun(*ops, nh).backward(o, st)
                got = {n: getattr(r, n).cpu(L, B, E) for n in ("gq", "gk", "gv")}
                bfam = bwd_family(L, hd)
            else:
                gq, gk, gv = K.attn_long_bwd(qd, kd, vd, o.view.unflatten(0, (L, B)), god, st, nh, False)
                torch.cuda.synchronize()
                got, bfam = {"gq": gq.cpu(), "gk": gk.cpu(), "gv": gv.cpu()}, "long"
            fam = "long" if "long" in (ffam, bfam) else bfam
            check_attn(f"head_dim {hd}, forward {fname} -> backward {bname}", got, ref, ref32, {n: fam for n in got}, ops, fails)
    assert not fails, fails


# ================================================================================================================================= LSTM
def lstm_ref(pre, whh, bhh, gout, dtype=torch.float64, whh_bf16=False):
    """the recurrence of a bidirectional LSTM from its input projection: pre [S, B, 2, 4H] (gate order i, f, g, o), whh [2, 4H, H],
    bhh [2, 4H], zero initial state, direction 1 walks t = S-1 .. 0 -> hout [S, B, 2H], gsav [S, B, 2, 4H] (gate activations),
    csav [S, B, 2, 2H] (c | tanh(c)), dG = d pre for the output gradient gout (autograd)"""
    S, B, _, H4 = pre.shape
    H = H4 // 4
    if whh_bf16:
        whh = whh.bfloat16().float()
    pre = pre.to(dtype).clone().requires_grad_(True)
    whh, bhh = whh.to(dtype), bhh.to(dtype)
    hs, gs, cs = [[None] * S, [None] * S], [[None] * S, [None] * S], [[None] * S, [None] * S]
    for d in range(2):
        h = torch.zeros(B, H, dtype=dtype)
        c = torch.zeros(B, H, dtype=dtype)
        for t in (range(S) if d == 0 else range(S - 1, -1, -1)):
            z = pre[t, :, d] + (h @ whh[d].t() + bhh[d])
            i, f, g, o = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), torch.sigmoid(z[:, 3 * H:])
            c = f * c + i * g
            tc = torch.tanh(c)
            h = o * tc
            hs[d][t], gs[d][t], cs[d][t] = h, torch.cat([i, f, g, o], 1), torch.cat([c, tc], 1)
    hout = torch.stack([torch.cat([hs[0][t], hs[1][t]], 1) for t in range(S)])
    hout.backward(gout.to(dtype))
    gsav = torch.stack([torch.stack([gs[0][t], gs[1][t]], 1) for t in range(S)]).detach()
    csav = torch.stack([torch.stack([cs[0][t], cs[1][t]], 1) for t in range(S)]).detach()
    return {"hout": hout.detach(), "gsav": gsav, "csav": csav, "dG": pre.grad, "bias": pre.grad.sum(dim=(0, 1))}


def lstm_operands(S, B, H, scale, seed):
    """pre ~ N(0, scale^2), whh, bhh ~ U(-1, 1) / sqrt(H) (torch's initialisation), gout ~ N(0, 1)"""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) / math.sqrt(H)     # noqa: E731
    return rnd(S, B, 2, 4 * H, seed=seed + 1, scale=scale), u(2, 4 * H, H), u(2, 4 * H), rnd(S, B, 2 * H, seed=seed + 2)


class Arena:
    """n floats between G NaN guards in a flat device buffer"""
    G = 64

    def __init__(self, n, fill=NAN):
        self.buf = torch.full((n + 2 * self.G,), NAN, device=DEV)
        self.t = self.buf[self.G:self.G + n]
        if isinstance(fill, torch.Tensor):
            self.t.copy_(fill.reshape(-1))
        else:
            self.t.fill_(fill)
        self.ptr = self.t.data_ptr()

    def guards_nan(self):
        return bool(torch.isnan(self.buf[:self.G]).all()) and bool(torch.isnan(self.buf[-self.G:]).all())

    def written(self):
        return self.guards_nan() and bool(torch.isfinite(self.t).all())

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


def lstm_family(H):
    return "st128" if H == 128 else "generic"


class LstmRun:
    def __init__(self, pre, whh, bhh, gout):
        self.S, self.B, self.H = pre.shape[0], pre.shape[1], pre.shape[3] // 4
        self.pre, self.whh, self.bhh, self.gout = (t.contiguous().to(DEV) for t in (pre, whh, bhh, gout))

    def dims(self):
        return self.S, self.B, self.H, stream()

    def forward(self, save=True):
        S, B, H = self.S, self.B, self.H
        self.hout = Arena(S * B * 2 * H)
        self.gsav = Arena(S * B * 8 * H) if save else None
        self.csav = Arena(S * B * 4 * H) if save else None
        _lib.call("fqss_lstm_fwd", self.pre.data_ptr(), self.whh.data_ptr(), self.bhh.data_ptr(), self.hout.ptr,
                  self.gsav.ptr if save else None, self.csav.ptr if save else None, *self.dims())
        torch.cuda.synchronize()
        assert self.hout.written() and (not save or (self.gsav.written() and self.csav.written())), "a NaN left inside or a guard overwritten"
        return self

    def fwd_outputs(self):
        S, B, H = self.S, self.B, self.H
        return {"hout": self.hout.t.cpu().view(S, B, 2 * H), "gsav": self.gsav.t.cpu().view(S, B, 2, 4 * H),
                "csav": self.csav.t.cpu().view(S, B, 2, 2 * H)}

    def backward(self, entry="fqss_lstm_bwd", gbias=None, gb4=None):
        """-> dG [S, B, 2, 4H] on the CPU; gbias: an Arena of [2][4H]; gb4: four device tensors [4H]"""
        dG = Arena(self.S * self.B * 8 * self.H)
        args = [self.gout.data_ptr(), self.whh.data_ptr(), self.gsav.ptr, self.csav.ptr, dG.ptr]
        if entry == "fqss_lstm_bwd_b":
            args.append(gbias.ptr)
        elif entry == "fqss_lstm_bwd_b4":
            args.append(K._ptr_array(list(gb4)))
        _lib.call(entry, *args, *self.dims())
        torch.cuda.synchronize()
        assert dG.written(), f"{entry}: a NaN left inside dG or a guard overwritten"
        return dG.t.cpu().view(self.S, self.B, 2, 4 * self.H)


def check_lstm(tag, got, ref, ref32, fam, fails):
    for name, g in got.items():
        b_elem, b_norm = LSTM_BOUND[fam][name]
        e_elem, e_norm = errs(g, ref[name])
        f_elem, f_norm = errs(ref32[name], ref[name])
        print(f"MEAS lstm {fam} {name} e_elem {e_elem:.2e} e_norm {e_norm:.2e} fp32 {f_elem:.2e} {f_norm:.2e} | {tag}")
        if not (bool(torch.isfinite(g).all()) and e_elem <= b_elem and e_norm <= b_norm):
            fails.append((tag, name, e_elem, e_norm, b_elem, b_norm))


class BiasSlots:
    """the four bias-gradient buffers b_ih, b_hh (forward), b_ih, b_hh (reverse) as [4H] slots of ONE arena with NaN gaps between them,
    started from random non-zero values of the sums' own size"""

    def __init__(self, H, start_scale, seed):
        self.n, self.gap = 4 * H, 16
        self.pitch = (self.n + self.gap + 3) // 4 * 4
        self.arena = torch.full((4 * self.pitch,), NAN, device=DEV)
        self.slots = [self.arena[i * self.pitch:i * self.pitch + self.n] for i in range(4)]
        for i, s in enumerate(self.slots):
            s.copy_(rnd(self.n, seed=seed + i, scale=start_scale))
        self.before = [s.cpu().double() for s in self.slots]

    def added(self):
        """after - before per slot; the gaps must still be NaN"""
        gaps = torch.ones_like(self.arena, dtype=torch.bool)
        for i in range(4):
            gaps[i * self.pitch:i * self.pitch + self.n] = False
        assert bool(torch.isnan(self.arena[gaps]).all()), "a write between the bias slots"
        return [s.cpu().double() - b for s, b in zip(self.slots, self.before)]


# (S, B, H, scale of pre)
LSTM_CASES = {
    "generic, H 1, B 2": (5, 2, 1, 1.0),
    "generic, H 3, B 3": (5, 3, 3, 1.0),
    "generic, H 4, B 3": (40, 3, 4, 1.0),
    "generic, H 4, B 2, S 2": (2, 2, 4, 1.0),
    "generic, H 12, B 7": (40, 7, 12, 1.0),
    "generic, H 12, B 2, S 1": (1, 2, 12, 1.0),
    "generic, H 64, B 1": (40, 1, 64, 1.0),
    "generic, H 64, B 2, S 250": (250, 2, 64, 1.0),
    "generic, H 100, B 1, S 1": (1, 1, 100, 1.0),
    "generic, H 100, B 2, S 2": (2, 2, 100, 1.0),
    "generic, H 100, B 3, S 40": (40, 3, 100, 1.0),
    "generic, H 100, B 7, S 250": (250, 7, 100, 1.0),
    "generic, H 100, B 2, saturated gates": (40, 2, 100, 20.0),
    "st<128>, H 128, B 1, S 1": (1, 1, 128, 1.0),
    "st<128>, H 128, B 2, S 2": (2, 2, 128, 1.0),
    "st<128>, H 128, B 3, S 40": (40, 3, 128, 1.0),
    "st<128>, H 128, B 7, S 250": (250, 7, 128, 1.0),
    "st<128>, H 128, B 2, S 500": (500, 2, 128, 1.0),
    "st<128>, H 128, B 3, saturated gates": (40, 3, 128, 20.0),
    "generic, H 200 (832 threads, 32 idle), B 3": (40, 3, 200, 1.0),
    "generic, H 200, B 2": (40, 2, 200, 1.0),
    "generic, H 256 (1024 threads), B 1": (40, 1, 256, 1.0),
    "generic, H 256, B 2": (40, 2, 256, 1.0),
}


@pytest.mark.parametrize("case", list(LSTM_CASES))
def test_lstm_against_fp64(case):
    """fqss_lstm_fwd and the three backward entries on a random input projection, so that the recurrence alone is measured, against
    float64: hout, the saved gate activations and cell states on the layout csrc/lstm.hip documents, dG = d pre, and the bias sums =
    the column sums of dG per direction, ADDED into buffers that start from random values (fqss_lstm_bwd_b: one [2][4H] buffer;
    fqss_lstm_bwd_b4: four slots of an arena, b_ih and b_hh of a direction receiving the same sums, the gaps untouched).  The
    inference form (gsav = csav = NULL) gives the same hout bit for bit; dG is bit-identical across the three entries and over two
    runs (one writer per element; the bias sums are fp32 atomics: only the float64 bound applies to them)."""
    S, B, H, scale = LSTM_CASES[case]
    fam = lstm_family(H)
    assert case.startswith("st<128>") == (fam == "st128")
    ops = lstm_operands(S, B, H, scale, seed=200 + H + S)
    ref, ref32 = lstm_ref(*ops), lstm_ref(*ops, dtype=torch.float32)
    fails = []
    run = LstmRun(*ops).forward()
    got = run.fwd_outputs()
    infer = LstmRun(*ops).forward(save=False)
    assert same_bits(infer.hout.t, run.hout.t), "the inference form's hout differs from the saving run's"
    again = LstmRun(*ops).forward().fwd_outputs()
    for n in got:
        assert same_bits(got[n], again[n]), f"{n}: two runs differ"
    dG = run.backward()
    assert same_bits(dG, run.backward()), "dG: two runs differ"
    got["dG"] = dG
    check_lstm(case, got, ref, ref32, fam, fails)
    bias_scale = rms(ref["bias"])
    # fqss_lstm_bwd_b: [2][4H], added
    gbias = Arena(8 * H, fill=rnd(8 * H, seed=5, scale=bias_scale))
    before = gbias.t.cpu().double()
    assert same_bits(run.backward("fqss_lstm_bwd_b", gbias=gbias), dG), "fqss_lstm_bwd_b: dG differs from fqss_lstm_bwd's"
    assert gbias.guards_nan()
    check_lstm(case + ", fqss_lstm_bwd_b", {"bias": (gbias.t.cpu().double() - before).view(2, 4 * H)}, ref, ref32, fam, fails)
    # fqss_lstm_bwd_b4: four slots
    slots = BiasSlots(H, bias_scale, seed=9)
    assert same_bits(run.backward("fqss_lstm_bwd_b4", gb4=slots.slots), dG), "fqss_lstm_bwd_b4: dG differs from fqss_lstm_bwd's"
    add = slots.added()
    for which, pair in (("b_ih", (add[0], add[2])), ("b_hh", (add[1], add[3]))):
        check_lstm(f"{case}, fqss_lstm_bwd_b4 {which}", {"bias": torch.stack(pair)}, ref, ref32, fam, fails)
    assert not fails, fails
    if S > 1 and scale == 1.0:
        mut = lstm_ref(*ops, whh_bf16=True)
        for name in ("hout", "dG"):
            floor = errs(mut[name], ref[name])[0]
            print(f"FLOOR lstm {name} whh rounded to bf16 {floor:.2e} | {case}")
            assert LSTM_BOUND[fam][name][0] * 10 <= floor, (case, name, floor)


def test_lstm_refuses_bad_arguments():
    """H = 0, H = 257, S = 0, B = 0, and exactly one of gsav / csav NULL: FQSS_EINVAL with a message naming the entry, nothing written"""
    S, B, H = 3, 2, 8
    run = LstmRun(*lstm_operands(S, B, H, 1.0, seed=1))
    hout, gsav, csav, dG, gbias = Arena(S * B * 2 * 257), Arena(S * B * 8 * 257), Arena(S * B * 4 * 257), Arena(S * B * 8 * 257), Arena(8 * 257)
    gb4 = K._ptr_array([gbias.t[i * 4 * H:(i + 1) * 4 * H] for i in range(4)])
    st = stream()
    fwd = [run.pre.data_ptr(), run.whh.data_ptr(), run.bhh.data_ptr(), hout.ptr, gsav.ptr, csav.ptr]
    bwd = [run.gout.data_ptr(), run.whh.data_ptr(), gsav.ptr, csav.ptr, dG.ptr]
    for dims in ((S, B, 0), (S, B, 257), (0, B, H), (S, 0, H), (S, B, -1)):
        refused("fqss_lstm_fwd", *fwd, *dims, st)
        refused("fqss_lstm_bwd", *bwd, *dims, st)
        refused("fqss_lstm_bwd_b", *bwd, gbias.ptr, *dims, st)
        refused("fqss_lstm_bwd_b4", *bwd, gb4, *dims, st)
    refused("fqss_lstm_fwd", *fwd[:4], None, csav.ptr, S, B, H, st)
    refused("fqss_lstm_fwd", *fwd[:4], gsav.ptr, None, S, B, H, st)
    refused("fqss_lstm_bwd_b", *bwd, None, S, B, H, st)
    for a in (hout, gsav, csav, dG, gbias):
        assert a.untouched()


@pytest.fixture
def det_off():
    yield
    K.DetMode.off()          # (the control block is device-wide: no later test may run under it)


@pytest.mark.parametrize("case", ["st<128>, H 128", "generic, H 100"])
def test_lstm_bias_sums_deterministic_mode(case, det_off):
    """FQSS_DETERMINISTIC=1 arithmetic (fqss_dev.h grad_add: integer sums on the shadow of the attached slot-0 arena, fqss_det_finish
    rounds once): the bias sums of fqss_lstm_bwd_b4 into four slices of that arena are bit-identical over two runs and meet the same
    float64 bound as the fp32-atomic path; dG does not depend on the mode."""
    H = 128 if "128" in case else 100
    S, B = 40, 7
    fam = lstm_family(H)
    ops = lstm_operands(S, B, H, 1.0, seed=300 + H)
    ref, ref32 = lstm_ref(*ops), lstm_ref(*ops, dtype=torch.float32)
    run = LstmRun(*ops).forward()
    dG = run.backward()
    start = rnd(4, 4 * H, seed=11, scale=rms(ref["bias"]))
    pitch = 4 * H + 32
    arena = torch.zeros(4 * pitch, device=DEV)
    slots = [arena[i * pitch:i * pitch + 4 * H] for i in range(4)]
    det = K.DetMode()
    det.attach(0, arena)
    det.activate()
    runs = []
    for _ in range(2):
        arena.zero_()
        for s, v in zip(slots, start):
            s.copy_(v)
        d = run.backward("fqss_lstm_bwd_b4", gb4=slots)
        det.finish(0)
        torch.cuda.synchronize()
        runs.append((d, arena.cpu().clone()))
    K.DetMode.off()
    assert same_bits(runs[0][0], dG) and same_bits(runs[1][0], dG), "dG depends on the deterministic mode"
    assert torch.equal(runs[0][1], runs[1][1]), "deterministic mode: the bias sums of two runs differ"
    a = runs[0][1]
    gaps = torch.ones_like(a, dtype=torch.bool)
    for i in range(4):
        gaps[i * pitch:i * pitch + 4 * H] = False
    assert bool((a[gaps] == 0).all()), "a write between the bias slots"
    add = [a[i * pitch:i * pitch + 4 * H].double() - start[i].double() for i in range(4)]
    fails = []
    for which, pair in (("b_ih", (add[0], add[2])), ("b_hh", (add[1], add[3]))):
        check_lstm(f"{case}, deterministic fqss_lstm_bwd_b4 {which}", {"bias": torch.stack(pair)}, ref, ref32, fam, fails)
    assert not fails, fails
