"""The q-GEMM kernels of csrc/qgemm.hip -- k_qgemm<0> (coded forward), k_qgemm<1, 3> (data gradient), k_qwgrad2 / k_qwgrad_group (weight
gradients), the float-operand modes 3 and 4 and k_wq_codes -- at the C ABI, against exact integers and float64.  The entry points are
called through fqss_amd._lib with explicit pointers and leading dimensions.

Entry points covered: fqss_wq_codes, fqss_wq_codes_bits, fqss_qpw_fwd, fqss_qpw_fwd2, fqss_qpw_fwdq (+ stats1), fqss_qpw_fwdq_add,
fqss_qpw_bwd_x, fqss_qpw_bwd_x_add, fqss_qpw_bwd_x2, fqss_qpw_bwd_w, fqss_qpw_bwd_w2, fqss_qpw_bwd_w_group, fqss_qpw_bwd_w_group_ws,
fqss_pwconv_fwd_x3, fqss_pwconv_fwd_x3s, fqss_pwconv_fwd_wq, and the deterministic-mode form of k_qwgrad2's fp32 atomics.  Every entry has
guarded-buffer cases and one refusal per FQSS_REQUIRE of its impl that the flat ABI can reach (test_*_refusals).  Not reachable there:
"fused AddQ: the conv in front of it has no activation" -- fqss_qpw_fwdq_add passes FQSS_ACT_NONE itself.

Layout under test.  fp32 operands sit in NaN-filled flat buffers between guard floats, row padding [M, ld) stays NaN; code operands sit in
0xA5-filled buffers between guard bytes (Cod below); outputs are NaN- / 0xA5-filled.  At least one operand of every case has padding
beyond the round-up its alignment rule asks for, and the operands of a case have different ld's.  After each call: every operand
bit-identical, the guards and everything outside what include/fqss.h lets the kernel write untouched -- fp32 outputs: columns >=
roundup4(M) of each row; code outputs: columns >= min(roundup64(M), ld) (whole 16-B granules of the last column tile); gw: nothing outside
its dense Co x Ci; the statistics slots and the group workspace: nothing outside their bytes -- and every live output element finite.

Exact-integer cases (torch.equal, no tolerance): with dw = 1, dx = 1 (range [lo, lo + 255], lo an integer) every term of every kernel
is an integer and the sum of the absolute products stays below 2^24 (asserted on the CPU, test_references_on_cpu and exact_ok()), so
fp32 gives the integer whatever the order.  The dgrad runs with gz = n 2^-s, |n| < 2^10 (K <= 64) and |n| < 2^17 (4-bit weight codes,
K = 16) reach the second and third bf16 piece of the split (asserted on the CPU on those operands); the wgrad run of that kind takes
|n| < 2^17 against codes 0 .. 3 at M = 33.

Forward against float64 with real ranges: the bound is derived, not measured -- the kernel forms the exact integer S, then
v = dw (dx S + min_x R) + b in at most five roundings (dx S, min_x R, their sum, dw x, + b): to first order 2^-24 (|dw dx S| +
|dw min_x R| + ...) each, FWD_ULPS = 6 of them covers the second-order terms: |z - ref| <= 6 2^-24 (|dw dx S| + |dw min_x R| + |b|) per
element, ref built from the integer S and R with dx the fp32 value of (hi - lo) / 255.

Measured on the MI355X (two runs; the sums of k_qwgrad2 go through fp32 atomics and differ from run to run): largest e_elem / e_norm
over a family's cases, beside torch fp32 on the CPU on the same cases, the bound (BOUND below) and its factor over the measurement:
                                         kernel               fp32                 bound                factor
  forward (all four entries)   z         <= 0.43 of the derived per-element bound (torch fp32 conv1d: up to 106 x that bound at Ci = 512)
  fqss_qpw_bwd_x / _add / _x2  gx        2.99e-6 / 3.43e-7    4.04e-6 / 5.84e-7    1.05e-5 / 1.2e-6     3.5 / 3.5   (Co = 1024, Ci = 512 + addend)
  fqss_qpw_bwd_w / _w2         gw        4.64e-6 / 3.52e-7    2.08e-6 / 2.71e-7    1.6e-5 / 1.2e-6      3.4 / 3.4   (M = 256 in one chain per tile;
                                                                                                        deterministic mode: 1.8e-6 / 3.4e-7)
  fqss_qpw_bwd_w_group         gw        3.06e-6 / 2.89e-7    2.08e-6 / 2.71e-7    1.05e-5 / 1e-6       3.4 / 3.5   (64-column stages summed in part order)
  fqss_pwconv_fwd_x3           z         3.18e-6 / 3.15e-7    2.33e-6 / 4.14e-7    1.1e-5 / 1.1e-6      3.5 / 3.5   (Ci = 432, Co = 512)
  fqss_pwconv_fwd_x3s          z         3.18e-6 / 3.17e-7    2.33e-6 / 4.14e-7    1.1e-5 / 1.1e-6      3.5 / 3.5   (the same case)
  fqss_pwconv_fwd_wq           z         2.65e-6 / 2.00e-7    4.20e-6 / 3.72e-7    9.2e-6 / 7e-7        3.5 / 3.5   (Ci = 432, Co = 512)
(e_elem is a maximum over heavy-tailed gradients divided by an rms: it sits an order above e_norm, for torch fp32 as for the kernels.)
Bit-exact, no bound: every exact-integer case; fqss_wq_codes(_bits) idx / idxT / dw / rw; fqss_qpw_fwdq's z against fqss_qpw_fwd and its
codes against oracle.act_indices of the activated z; the statistics slots; fqss_qpw_fwdq_add's sum codes against fqss_ewq_fwd; Co = 1536
in two parts against two launches summed on the host; fqss_qpw_bwd_w_group run to run; deterministic mode run to run.
fqss_qpw_fwdq_add against a float64 evaluation of fq(dec(a) + dec(y)): at most one level off on at most ADD_SHARE = 2e-4 of the codes
(the cap of tests/test_gpu_norm_kernels.py); torch fp32 on the CPU on the same operands is asserted inside the same cap.

Mutation floors: e_elem of the wrong kernel, computed in float64 on the CPU on each case's own operands, asserted 10 x above the bound
in every non-void case of every run (floor() below; for the forward the unit is the derived per-element bound).
Smallest floor over the non-void cases (the forward's in units of the element's bound, where 10 is asked):
  forward   last k-tile dropped 5.0e6 (void at Ci <= 32: one tile); min_x R dropped 7.9e5; dw of the neighbouring row 3.3e6 (void at
            Co = 1); pair split one row off (the two rows at the split take the other layer's bias) 6.5e5 (pairs with bias); the addend
            dropped (fqss_qpw_fwdq_add): more than one level off on > 10 x ADD_SHARE of the codes.  Void: last batch dropped -- the
            batches are separate outputs, an unwritten one stays NaN and fails the finite check
  dgrad     last k-tile dropped 0.43 (void at Co = 16); dw of the neighbouring row 0.82; pair split one row off 4.4; the addend dropped
            0.29; second part of a Co > 1024 reduction dropped 2.3
  wgrad     (both kernels) last 64-column stage dropped 0.27 (void at M <= 64); min_x rowsum dropped 0.60; pair split one row off 4.1;
            last live column dropped 0.22 (void at M = 1); padding column M read as a gz of the case's rms (1.0 would be 1000 x that)
            against code 255: 6.2e-2 (M = 1030, the most diluted case); last batch dropped 2.5 (B > 1)
  float     last k-tile dropped (Ci <= 32: the last four k) 0.31; bias dropped 0.45; coded weight: last k-tile 1.1, dw of the
            neighbouring row 2.6
  Void in the float64 cases: the third bf16 piece of gz dropped.  It moves a product by at most 2^-16 of itself: e_elem 3.7e-6 .. 1.1e-4
  and e_norm 3.7e-6 .. 1.1e-5 on these operands (printed per case) -- over the bounds, so a library without the piece fails the float64
  cases of both gradients, but by a factor 3 to 9 (e_norm), not the 10 asked of a floor.
  The bit-exact runs hold it instead: test_dgrad_exact_through_the_bf16_pieces and test_wgrad_exact_through_the_bf16_pieces assert on
  the CPU that their operands have non-zero second and third pieces and that a kernel without the piece differs (differs() below), and
  every other exact-integer case asserts a differing element count for an index one off, the last column / batch / min_x term dropped.

Checked once on the MI355X against scratch copies of the library carrying ONE arithmetic mutation each (built outside the package, never
committed; every copy fails this file): the mask k + e < kend on gz dropped in both wgrad kernels -- 27 tests fail (the NaN padding
reaches gw); the third bf16 piece dropped in k_qgemm<1> and k_qwgrad2 -- 26 (both piece tests, every float64 gradient case); B rows past
K not zeroed in the forward -- 13 (every exact and float64 case with Ci % 32 = 16); the statistics taken over padding positions too -- 4.

Defects found and fixed with this file:
  1. fqss_qpw_fwdq accepted a non-null stats1 for a shape whose fqss_qpw_stat_slots(Co1, M) is 0 (more than 1024 tiles): the kernel then
     wrote B x tiles slots into a buffer the header sizes at zero bytes.  The descriptor form guarded it, the flat entry did not: it now
     returns FQSS_EINVAL in front of the launch (test_forward_refusals).  Measured for Co1 = 1, M = 65 600 with full-size buffers: the
     library of the parent commit returns FQSS_OK and writes 1025 slots; now FQSS_EINVAL, no slot, z and the codes untouched.

References: plain float64 torch on the CPU from the formulas in the header comment of csrc/qgemm.hip; test_references_on_cpu ties them
to float64 F.conv1d on oracle.fqss_oracle.weight_quantize / act_quantize operands and to that graph's autograd.  e_elem = max |got - ref|
/ rms(ref), e_norm = ||got - ref|| / ||ref||; the yardstick is the same operation in torch fp32 on the CPU ("MEAS" lines)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import oracle.fqss_oracle as O
import tests.test_gpu_layout_spectral_kernels as L
from tests.test_gpu_layout_spectral_kernels import (DEV, EINVAL, F64, G, NAN, Blk, Vec, all_unchanged, errs, gpu, pad4, refused, rms,  # noqa: F401
                                                    stream)

K = None
_lib = None
GB = 256                                 # guard bytes on either side of every code buffer
SENT = 0xA5                              # what code buffers are filled with (as a code: 165, finite)
ISENT = -7777                            # ... and the int64 statistics slots
ACT_NONE, ACT_PRELU, ACT_RELU = 0, 1, 2
ULP = 2.0 ** -24
FWD_ULPS = 6.0                           # derived (see above)
ADD_SHARE = 2e-4
TWO24 = float(1 << 24)

# per family and tensor: (e_elem bound, e_norm bound), at most 4 x the largest figure measured on the MI355X over the family's cases
BOUND = {
    "dgrad": {"gx": (1.05e-5, 1.2e-6)},
    "wgrad": {"gw": (1.6e-5, 1.2e-6)},
    "group": {"gw": (1.05e-5, 1e-6)},
    "x3": {"z": (1.1e-5, 1.1e-6)},
    "x3s": {"z": (1.1e-5, 1.1e-6)},
    "wq": {"z": (9.2e-6, 7e-7)},
}


@pytest.fixture(scope="module")
def _gpu():
    global K, _lib
    L._gpu_fixture()
    K, _lib = L.K, L._lib
    yield


def r4(n):
    return (n + 3) // 4 * 4


def r16(n):
    return (n + 15) // 16 * 16


def gen(seed):
    return torch.Generator().manual_seed(seed)


def sync():
    torch.cuda.synchronize()


def call(name, *args):
    _lib.call(name, *args)
    sync()


# ------------------------------------------------------------------------------------------------------------------------- buffers
class Cod:
    """[R][M] bytes (u8 or int8 codes) with row stride ld, `off` bytes into a SENT-filled flat device buffer that begins and ends with GB
    guard bytes (the buffer is 256-B aligned: the base is 16-B aligned iff off % 16 == 0).  fill: an operand (its buffer is snapshot for
    unchanged()); without it an output"""

    def __init__(self, R, M, ld=None, off=0, fill=None):
        ld = M if ld is None else ld
        assert ld >= M
        self.R, self.M, self.ld, self.o = R, M, ld, GB + off
        self.buf = torch.full((self.o + R * ld + GB,), SENT, dtype=torch.uint8, device=DEV)
        assert self.buf.data_ptr() % 256 == 0
        self.view = self.buf.as_strided((R, M), (ld, 1), self.o)
        self.ptr = self.buf.data_ptr() + self.o
        self.before = None
        if fill is not None:
            self.view.copy_(fill.reshape(R, M).contiguous().view(torch.uint8))
            self.before = self.buf.clone()

    def unchanged(self):
        return bool(torch.equal(self.buf, self.before))

    def written(self, wcols=None):
        """the guards and every byte outside columns [0, min(wcols, ld)) of the rows still hold SENT"""
        w = self.M if wcols is None else min(wcols, self.ld)
        keep = torch.ones_like(self.buf, dtype=torch.bool)
        keep.as_strided((self.R, w), (self.ld, 1), self.o).fill_(False)
        return bool((self.buf[keep] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())

    def cpu(self, *shape, signed=False):
        t = self.view.cpu().contiguous()
        t = t.view(torch.int8) if signed else t
        return t.reshape(*shape) if shape else t


class Slots:
    """n int64 between G guards, ISENT-filled (the statistics slots of fqss_qpw_fwdq)"""

    def __init__(self, n):
        self.buf = torch.full((n + 2 * G,), ISENT, dtype=torch.int64, device=DEV)
        self.t = self.buf[G:G + n]
        self.ptr = self.t.data_ptr()

    def guards(self):
        return bool((self.buf[:G] == ISENT).all()) and bool((self.buf[-G:] == ISENT).all())

    def untouched(self):
        return bool((self.buf == ISENT).all())


def fwritten(blk):
    """an fp32 output: [0, M) of every row finite; the guards and everything outside columns [0, roundup4(M)) of the rows still NaN"""
    w = min(r4(blk.M), blk.ld)
    keep = torch.ones_like(blk.buf, dtype=torch.bool)
    keep.as_strided((blk.R, w), (blk.ld, 1), blk.o).fill_(False)
    return bool(torch.isfinite(blk.view).all()) and bool(torch.isnan(blk.buf[keep]).all())


def sc(v):
    """a device scalar (a quantizer range, a slope) between guards"""
    return Vec(1, fill=float(v))


def f32(v):
    return torch.tensor([v], dtype=torch.float32)


def delta32(lo, hi):
    """the fp32 step of an activation range, as load_qrange / the epilogues form it: (hi - lo) / 255 in fp32"""
    return (f32(hi) - f32(lo)) / 255.0


# ----------------------------------------------------------------------------------------------------------------- operands (CPU)
def codes(g, *shape):
    c = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    c.view(-1)[0], c.view(-1)[-1] = 0, 255
    return c


def wcodes(g, Co, Ci, lim=128):
    w = torch.randint(-lim, lim, (Co, Ci), generator=g, dtype=torch.int8)
    w.view(-1)[0], w.view(-1)[-1] = -lim, lim - 1
    return w


def ints(g, lim, *shape):
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


def heavy(g, *shape, scale=1e-3):
    """heavy-tailed like real gradients (tests/test_gpu_kernels.py::test_gradient_gemms_exact_split)"""
    return torch.randn(*shape, generator=g) * torch.exp(torch.randn(*shape, generator=g)) * scale


def steps(g, Co):
    return torch.rand(Co, generator=g) * 2e-3 + 5e-4


def split3(gz):
    """the exact three bf16 pieces of qgemm.hip's split3 (truncations)"""
    tr = lambda t: (t.contiguous().view(torch.int32) & -65536).view(torch.float32)
    h1 = tr(gz)
    r1 = gz - h1
    h2 = tr(r1)
    return h1, h2, r1 - h2


def exact_ok(*abs_sums):
    """an exact-integer construction: the sum of the absolute values of every term stays below 2^24, so fp32 is exact in any order"""
    return all(float(a.double().max()) < TWO24 for a in abs_sums)


# ------------------------------------------------------------------------------------------------------------- references (float64)
def fwd_parts(wi, c, dw, bias, lo, hi):
    """S, R, and the three terms of z = dw (dx S + min_x R) + b in float64; dx is the fp32 step"""
    S = torch.einsum("oc,bcm->bom", wi.double(), c.double())
    R = wi.double().sum(1)
    dx, mn = delta32(lo, hi).double(), f32(lo).double()
    t1 = dw.double()[None, :, None] * dx * S
    t2 = (dw.double() * mn * R)[None, :, None].expand_as(S)
    t3 = (bias.double() if bias is not None else torch.zeros(wi.shape[0], dtype=F64))[None, :, None].expand_as(S)
    return S, R, t1, t2, t3


def fwd_ref(wi, c, dw, bias, lo, hi):
    _, _, t1, t2, t3 = fwd_parts(wi, c, dw, bias, lo, hi)
    return t1 + t2 + t3


def fwd_bound(wi, c, dw, bias, lo, hi):
    _, _, t1, t2, t3 = fwd_parts(wi, c, dw, bias, lo, hi)
    return FWD_ULPS * ULP * (t1.abs() + t2.abs() + t3.abs())


def dgrad_ref(wi, dw, gz, addend=None):
    """gx[b] = W_q^T gz[b] (+ addend), W_q = dw[co] Wi[co][ci]"""
    gx = torch.einsum("oc,bom->bcm", wi.double() * dw.double()[:, None], gz.double())
    return gx + addend.double() if addend is not None else gx


def wgrad_ref(gz, c, lo, hi, dropmin=False):
    """gw[co][ci] = sum_{b, m} gz (dx c + min_x)"""
    dx, mn = delta32(lo, hi).double(), f32(lo).double()
    gw = dx * torch.einsum("bom,bcm->oc", gz.double(), c.double())
    return gw if dropmin else gw + mn * gz.double().sum((0, 2))[:, None]


def pw_ref(w, x, bias):
    z = torch.einsum("oc,bcm->bom", w.double(), x.double())
    return z + bias.double()[None, :, None] if bias is not None else z


def measure(fam, name, got, ref, ref32, tag, fails):
    e_elem, e_norm = errs(got, ref)
    f_elem, f_norm = errs(ref32, ref) if ref32 is not None else (NAN, NAN)
    bound = BOUND[fam][name]
    print(f"MEAS {fam} {name} e_elem {e_elem:.2e} e_norm {e_norm:.2e} fp32 {f_elem:.2e} {f_norm:.2e} bound {bound[0]:.1e} {bound[1]:.1e} | {tag}")
    if not (e_elem <= bound[0] and e_norm <= bound[1]):
        fails.append((tag, name, e_elem, e_norm, bound))


def floor(fam, name, mut, ref, what, tag):
    """the bound stays 10 x below what the wrong kernel `what` gives on this case's operands"""
    fl = errs(mut, ref)[0]
    b = BOUND[fam][name][0]
    print(f"FLOOR {fam} {name} {what} {fl:.2e} (bound {b:.1e}) | {tag}")
    assert b * 10 <= fl, (tag, what, name, fl, b)


def floor_fwd(mut, ref, bnd, what, tag):
    """forward: the wrong kernel `what` misses the derived per-element bound by 10 x somewhere"""
    fl = float(((mut - ref).abs() / bnd.clamp_min(1e-300)).max())
    print(f"FLOOR fwd z {what} {fl:.2e} x the element's bound | {tag}")
    assert fl >= 10, (tag, what, fl)


def differs(mut, ref, what, tag):
    n = int((mut.double() != ref.double()).sum())
    print(f"FLOOR exact {what}: {n} of {ref.numel()} elements differ | {tag}")
    assert n > 0, (tag, what)


# ================================================================================================================== 1. weight codes
WQ_CASES = [(1, 16, 8), (33, 300, 4), (512, 512, 8), (33, 16, 2), (1, 300, 2), (512, 16, 4), (33, 512, 8)]


def wq_operands(Co, Ci, n_bits, seed):
    g = gen(seed)
    w = torch.randn(Co, Ci, generator=g) * 0.1
    lo = -(torch.rand(Co, generator=g) * 0.2 + 0.05)
    hi = torch.rand(Co, generator=g) * 0.2 + 0.05
    return w, lo, hi


def wq_run(w, lo, hi, n_bits, bits_entry=True):
    Co, Ci = w.shape
    wb, lob, hib = Blk(Co, Ci, fill=w), Vec(Co, fill=lo), Vec(Co, fill=hi)
    idx, idxT, dw, rw = Cod(Co, Ci), Cod(Ci, Co), Vec(Co), Vec(Co)
    if bits_entry:
        call("fqss_wq_codes_bits", wb.ptr, idx.ptr, idxT.ptr, dw.ptr, rw.ptr, Co, Ci, lob.ptr, hib.ptr, n_bits, stream())
    else:
        call("fqss_wq_codes", wb.ptr, idx.ptr, idxT.ptr, dw.ptr, rw.ptr, Co, Ci, lob.ptr, hib.ptr, stream())
    all_unchanged(w=wb, lo=lob, hi=hib)
    assert idx.written() and idxT.written() and dw.written() and rw.written()
    return idx.cpu(signed=True), idxT.cpu(signed=True), dw.cpu(), rw.cpu()


@gpu
@pytest.mark.parametrize("Co,Ci,n_bits", WQ_CASES)
def test_weight_codes(Co, Ci, n_bits):
    """fqss_wq_codes_bits (and fqss_wq_codes at 8 bits): idx against the oracle, idxT its transpose, dw the fp32 step bit for bit, rw the
    exact integer row sum"""
    w, lo, hi = wq_operands(Co, Ci, n_bits, Co + Ci + n_bits)
    want = O.weight_indices(w[:, :, None], lo[:, None, None], hi[:, None, None], n_bits)[:, :, 0]
    dw_ref = 2 * torch.maximum(lo.abs(), hi.abs()) / (2 ** n_bits - 1)
    for bits_entry in ((True, False) if n_bits == 8 else (True,)):
        idx, idxT, dw, rw = wq_run(w, lo, hi, n_bits, bits_entry)
        assert torch.equal(idx, want) and torch.equal(idxT, want.t())
        assert torch.equal(dw, dw_ref)
        assert torch.equal(rw.double(), want.double().sum(1))
        assert int(idx.min()) >= -2 ** (n_bits - 1) and int(idx.max()) <= 2 ** (n_bits - 1) - 1
    differs(want.roll(1, 1), want, "column index one off", f"wq {Co}x{Ci} {n_bits} bits")


@gpu
def test_weight_codes_refusals():
    Co, Ci = 4, 16
    w, lo, hi = wq_operands(Co, Ci, 8, 0)
    wb, lob, hib = Blk(Co, Ci, fill=w), Vec(Co, fill=lo), Vec(Co, fill=hi)
    idx, idxT, dw, rw = Cod(Co, Ci), Cod(Ci, Co), Vec(Co), Vec(Co)
    good = [wb.ptr, idx.ptr, idxT.ptr, dw.ptr, rw.ptr, Co, Ci, lob.ptr, hib.ptr]
    for bits in (1, 9):
        refused("fqss_wq_codes_bits", *good, bits, stream())
    for k in (0, 1, 2, 3, 4, 7, 8):
        a = list(good)
        a[k] = None
        refused("fqss_wq_codes_bits", *a, 8, stream())
        refused("fqss_wq_codes", *a, stream(), who="fqss_wq_codes")
    refused("fqss_wq_codes_bits", *good[:5], 0, Ci, *good[7:], 8, stream())
    assert idx.untouched() and idxT.untouched() and dw.untouched() and rw.untouched()


# ==================================================================================================================== 2. forward
# (B, Ci, Co1, Co2, M, bias).  Workgroups = B ceil(M / 64) ceil(Co / 128): 1 (first case) ... 36 (> 8, no multiple of 8)
FWD_CASES = [(1, 16, 1, 0, 1, False), (3, 48, 33, 0, 3, True), (1, 128, 130, 0, 63, True), (3, 512, 512, 0, 130, False),
             (1, 16, 512, 0, 64, True), (3, 128, 33, 0, 65, True), (1, 48, 130, 0, 130, False), (1, 512, 40, 24, 65, True),
             (3, 16, 16, 16, 130, False), (1, 128, 128, 128, 64, True), (3, 48, 96, 32, 3, True)]
# (B, Ci, Co1, Co2, M, act, stats)
FWDQ_CASES = [(3, 48, 33, 0, 3, ACT_PRELU, True), (1, 128, 130, 0, 63, ACT_RELU, True), (1, 16, 512, 0, 64, ACT_NONE, True),
              (3, 512, 512, 0, 130, ACT_PRELU, True), (1, 128, 128, 128, 64, ACT_NONE, False), (3, 48, 96, 32, 65, ACT_RELU, False),
              (1, 16, 1, 0, 130, ACT_NONE, True)]
# (B, Ci, Co1, Co2, M, which: bit 0 = an AddQ behind output 1, bit 1 = behind output 2)
FWDA_CASES = [(1, 128, 128, 128, 64, 3), (3, 48, 96, 32, 65, 2), (3, 16, 33, 0, 130, 1), (1, 512, 64, 64, 130, 1)]


def fwd_operands(B, Ci, Co1, Co2, M, bias, mode, seed):
    """mode "int": dw = 1, range [0, 255], integer bias; "min": the same with range [-3, 252]; "ext": every Wi = -128, every c = 255;
    "real": real steps and ranges"""
    g = gen(seed)
    Co = Co1 + Co2
    wi, c = wcodes(g, Co, Ci), codes(g, B, Ci, M)
    if mode == "ext":
        wi, c = torch.full_like(wi, -128), torch.full_like(c, 255)
    if mode == "real":
        dw, lo, hi = steps(g, Co), -0.731, 1.913
        b = torch.randn(Co, generator=g) if bias else None
    else:
        dw, (lo, hi) = torch.ones(Co), ((-3.0, 252.0) if mode == "min" else (0.0, 255.0))
        b = ints(g, 1000, Co) if bias else None
    return wi, c, dw, b, lo, hi


class FwdOps:
    """the device operands of one forward case: xc [B][Ci][ld_xc] with 16 bytes of padding beyond the round-up"""

    def __init__(self, B, Ci, Co1, Co2, M, wi, c, dw, b, lo, hi):
        self.dims = (B, Ci, Co1, Co2, M)
        Co = Co1 + Co2
        self.xc = Cod(B * Ci, M, r16(M) + 16, fill=c)
        self.wi = Cod(Co, Ci, fill=wi)
        self.dw, self.rw = Vec(Co, fill=dw), Vec(Co, fill=wi.double().sum(1))
        self.b1 = Vec(Co1, fill=b[:Co1]) if b is not None else None
        self.b2 = Vec(Co2, fill=b[Co1:]) if b is not None and Co2 else None
        self.lo, self.hi = sc(lo), sc(hi)

    def unchanged(self):
        ops = dict(xc=self.xc, wi=self.wi, dw=self.dw, rw=self.rw, lo=self.lo, hi=self.hi)
        ops.update({k: v for k, v in (("b1", self.b1), ("b2", self.b2)) if v is not None})
        all_unchanged(**ops)

    def head(self):
        p = lambda v: v.ptr if v is not None else None
        return [self.xc.ptr, self.wi.ptr, self.dw.ptr, self.rw.ptr, p(self.b1), p(self.b2), self.lo.ptr, self.hi.ptr]

    def zs(self):
        B, Ci, Co1, Co2, M = self.dims
        return Blk(B * Co1, M, pad4(M)), (Blk(B * Co2, M, r4(M) + 12) if Co2 else None)

    def plain(self):
        """fqss_qpw_fwd / fqss_qpw_fwd2 -> (z1, z2) on the CPU"""
        B, Ci, Co1, Co2, M = self.dims
        z1, z2 = self.zs()
        h = self.head()
        if Co2:
            call("fqss_qpw_fwd2", *h, z1.ptr, z2.ptr, B, Ci, Co1, Co2, M, self.xc.ld, z1.ld, z2.ld, stream())
        else:
            call("fqss_qpw_fwd", *h[:5], *h[6:], z1.ptr, B, Ci, Co1, M, self.xc.ld, z1.ld, stream())
        self.unchanged()
        assert fwritten(z1) and (z2 is None or fwritten(z2))
        return z1.cpu(B, Co1, M), (z2.cpu(B, Co2, M) if Co2 else None)

    def quant(self, act, slope, r1, r2, stats=False, adds=(None, None)):
        """fqss_qpw_fwdq (adds: fqss_qpw_fwdq_add) -> z1, z2, yc1, yc2, slots [B][n][2] | None, (sum codes 1, 2)"""
        B, Ci, Co1, Co2, M = self.dims
        z1, z2 = self.zs()
        y1, y2 = Cod(B * Co1, M, r16(M)), (Cod(B * Co2, M, r16(M) + 32) if Co2 else None)
        rs = [sc(v) for v in r1] + ([sc(v) for v in r2] if Co2 else [None, None])
        sl = sc(slope) if slope is not None else None
        p = lambda v: v.ptr if v is not None else None
        n = _lib.query("fqss_qpw_stat_slots", Co1, M) if stats else 0
        st = Slots(B * n * 2) if stats else None
        dims = [B, Ci, Co1, Co2, M, self.xc.ld, z1.ld, p(z2) and z2.ld or 0, y1.ld, p(y2) and y2.ld or 0]
        keep, souts = [], [None, None]
        if adds == (None, None):
            call("fqss_qpw_fwdq", *self.head(), z1.ptr, p(z2), act, p(sl), *[p(v) for v in rs], y1.ptr, p(y2), *dims, p(st), stream())
        else:
            ptrs = []
            for i, (ad, Co) in enumerate(zip(adds, (Co1, Co2))):
                if ad is None:
                    ptrs.append(None)
                    continue
                s = _lib.FqssAddAfter()
                souts[i] = Cod(B * Co, M, r16(M) + 16 * (2 - i))
                s.a, s.ld_a, s.amin, s.amax, s.qmin, s.qmax = ad["a"].ptr, ad["a"].ld, ad["alo"].ptr, ad["ahi"].ptr, ad["qlo"].ptr, ad["qhi"].ptr
                s.y, s.ld_y = souts[i].ptr, souts[i].ld
                keep.append(s)
                ptrs.append(ctypes.addressof(s))
            call("fqss_qpw_fwdq_add", *self.head(), z1.ptr, p(z2), *[p(v) for v in rs], y1.ptr, p(y2), *dims, *ptrs, stream())
            for ad in adds:
                if ad is not None:
                    all_unchanged(**ad)
        self.unchanged()
        all_unchanged(**{f"r{i}": v for i, v in enumerate(rs + [sl]) if v is not None})
        assert fwritten(z1) and (z2 is None or fwritten(z2))
        w64 = (M + 63) // 64 * 64
        assert y1.written(w64) and (y2 is None or y2.written(w64)) and all(s is None or s.written(w64) for s in souts)
        slots = None
        if stats:
            assert st.guards() and n > 0
            slots = st.t.cpu().reshape(B, n, 2)
        self.dev = dict(y1=y1, y2=y2, rs=rs)         # (kept for fqss_ewq_fwd on the same buffers)
        return (z1.cpu(B, Co1, M), z2.cpu(B, Co2, M) if Co2 else None, y1.cpu(B, Co1, M), y2.cpu(B, Co2, M) if Co2 else None, slots,
                tuple(s.cpu(B, Co, M) if s is not None else None for s, Co in zip(souts, (Co1, Co2))), souts)


def fwd_exact(case, mode, seed):
    B, Ci, Co1, Co2, M, bias = case
    wi, c, dw, b, lo, hi = fwd_operands(B, Ci, Co1, Co2, M, bias, mode, seed)
    S, R, t1, t2, t3 = fwd_parts(wi, c, dw, b, lo, hi)
    absS = torch.einsum("oc,bcm->bom", wi.double().abs(), c.double())
    assert float(delta32(lo, hi)) == 1.0 and exact_ok(absS + (abs(lo) * wi.double().abs().sum(1))[None, :, None] + t3.abs())
    ops = FwdOps(B, Ci, Co1, Co2, M, wi, c, dw, b, lo, hi)
    z1, z2 = ops.plain()
    ref = (t1 + t2 + t3).float()
    assert torch.equal(z1, ref[:, :Co1]), (case, mode)
    assert Co2 == 0 or torch.equal(z2, ref[:, Co1:]), (case, mode)
    return wi, c, ref


@gpu
@pytest.mark.parametrize("case", FWD_CASES, ids=str)
def test_forward_exact_integers(case):
    """fqss_qpw_fwd / fqss_qpw_fwd2 with dw = 1, dx = 1, min_x = 0 and integer bias: z is the int64 sum, bit for bit"""
    B, Ci, Co1, Co2, M, bias = case
    wi, c, ref = fwd_exact(case, "int", 100 + Ci + Co1 + M)
    tag = f"fwd exact {case}"
    if Ci > 1:
        differs(torch.einsum("oc,bcm->bom", wi.double().roll(1, 1), c.double()), torch.einsum("oc,bcm->bom", wi.double(), c.double()),
                "k index one off", tag)


@gpu
def test_forward_exact_integers_extreme_and_offset():
    """every Wi = -128, every c = 255 at Ci = 512: |S| = 16 711 680 < 2^24; and an integer min_x = -3 (range [-3, 252]: dx = 1), Ci <= 128"""
    fwd_exact((1, 512, 130, 0, 65, True), "ext", 1)
    fwd_exact((3, 512, 40, 24, 3, False), "ext", 2)
    fwd_exact((3, 128, 33, 0, 65, True), "min", 3)
    fwd_exact((1, 48, 96, 32, 130, True), "min", 4)
    fwd_exact((1, 16, 16, 16, 63, False), "min", 5)


@gpu
@pytest.mark.parametrize("case", FWD_CASES, ids=str)
def test_forward_against_fp64(case):
    """real steps and ranges: every element within 6 x 2^-24 (|dw dx S| + |dw min_x R| + |b|) of the float64 value"""
    B, Ci, Co1, Co2, M, bias = case
    Co = Co1 + Co2
    wi, c, dw, b, lo, hi = fwd_operands(B, Ci, Co1, Co2, M, bias, "real", 200 + Ci + Co1 + M)
    ops = FwdOps(B, Ci, Co1, Co2, M, wi, c, dw, b, lo, hi)
    z1, z2 = ops.plain()
    z = torch.cat([z1, z2], 1) if Co2 else z1
    S, R, t1, t2, t3 = fwd_parts(wi, c, dw, b, lo, hi)
    ref, bnd = t1 + t2 + t3, fwd_bound(wi, c, dw, b, lo, hi)
    x32 = delta32(lo, hi) * c.float() + f32(lo)
    z32 = F.conv1d(x32, (dw[:, None] * wi.float())[:, :, None], b)
    tag = f"fwd {case}"
    worst, worst32 = float(((z.double() - ref).abs() / bnd).max()), float(((z32.double() - ref).abs() / bnd).max())
    print(f"MEAS fwd z {worst:.2f} of the element's bound, torch fp32 {worst32:.2f} | {tag}")
    assert worst <= 1.0, (tag, worst)
    # mutation floors, in units of the element's bound
    kl = (Ci - 1) // 32 * 32
    if kl > 0:
        floor_fwd(fwd_ref(wi[:, :kl], c[:, :kl], dw, b, lo, hi), ref, bnd, "last k-tile dropped", tag)
    floor_fwd(t1 + t3, ref, bnd, "min_x R dropped", tag)
    if Co > 1:
        floor_fwd(fwd_ref(wi, c, dw.roll(1), b, lo, hi), ref, bnd, "dw of the neighbouring row", tag)
    if Co2 and b is not None:
        b1 = torch.cat([b[:Co1 - 1], b[Co1:Co1 + 1], b[Co1 - 1:Co1], b[Co1 + 1:]])       # the rows next to the split take the other layer's bias
        floor_fwd(fwd_ref(wi, c, dw, b1, lo, hi), ref, bnd, "pair split one row off", tag)


def act_cpu(z, act, slope):
    return z if act == ACT_NONE else torch.where(z > 0, z, z * (slope if act == ACT_PRELU else 0.0))


def out_range(t):
    """an output range both ends of which saturate: the quartiles of the activated z (integer-free fp32 values)"""
    q = torch.quantile(t.flatten().double(), torch.tensor([0.25, 0.75], dtype=F64))
    lo, hi = float(f32(float(q[0]))), float(f32(float(q[1])))
    return (lo, hi) if hi > lo else (lo - 0.5, lo + 0.5)


@gpu
@pytest.mark.parametrize("case", FWDQ_CASES, ids=str)
def test_forward_fused_quantizer(case):
    """fqss_qpw_fwdq: z bit-equal to the plain forward, codes bit-equal to oracle.act_indices of the activated kernel z, the statistics
    slots sum to the exact integer sum c / sum c^2 over the live positions"""
    B, Ci, Co1, Co2, M, act, stats = case
    wi, c, dw, b, lo, hi = fwd_operands(B, Ci, Co1, Co2, M, True, "real", 300 + Ci + Co1 + M)
    ops = FwdOps(B, Ci, Co1, Co2, M, wi, c, dw, b, lo, hi)
    p1, p2 = ops.plain()
    slope = 0.2 if act == ACT_PRELU else None
    r1 = out_range(act_cpu(p1, act, 0.2))
    r2 = out_range(act_cpu(p2, act, 0.2)) if Co2 else None
    z1, z2, y1, y2, slots, _, _ = ops.quant(act, slope, r1, r2, stats)
    for z, p, y, r in ((z1, p1, y1, r1), (z2, p2, y2, r2)):
        if z is None:
            continue
        assert torch.equal(z, p)
        want = O.act_indices(act_cpu(z, act, f32(0.2)), f32(r[0]), f32(r[1]))
        assert torch.equal(y, want), (case, int((y != want).sum()))
        if y.numel() >= 8:
            assert int(y.min()) == 0 and int(y.max()) == 255
    if stats:
        tot = slots.sum(1)
        assert torch.equal(tot[:, 0], y1.long().sum((1, 2))) and torch.equal(tot[:, 1], (y1.long() ** 2).sum((1, 2)))


@gpu
@pytest.mark.parametrize("case", FWDA_CASES, ids=str)
def test_forward_fused_adds(case):
    """fqss_qpw_fwdq_add: z and codes of fqss_qpw_fwdq, sum codes bit-equal to fqss_ewq_fwd on the same buffers and within one level of
    a float64 evaluation of fq(dec(a) + dec(y)) on all but ADD_SHARE of the codes"""
    B, Ci, Co1, Co2, M, which = case
    g = gen(400 + Ci + Co1 + M)
    wi, c, dw, b, lo, hi = fwd_operands(B, Ci, Co1, Co2, M, True, "real", 400 + Ci + Co1 + M)
    ops = FwdOps(B, Ci, Co1, Co2, M, wi, c, dw, b, lo, hi)
    p1, p2 = ops.plain()
    rng = lambda t: (float(f32(float(t.min()))), float(f32(float(t.max()))))
    r1, r2 = rng(p1), (rng(p2) if Co2 else None)
    adds, host = [], []
    for i, (Co, r) in enumerate(((Co1, r1), (Co2, r2))):
        if not (which >> i) & 1:
            adds.append(None)
            host.append(None)
            continue
        a = codes(g, B, Co, M)
        alo, ahi = -2.3 + i, 1.9 + i
        span = (ahi - alo) + (r[1] - r[0])
        qlo, qhi = alo + r[0] + 0.2 * span, ahi + r[1] - 0.3 * span          # the sum saturates at both ends in places
        adds.append(dict(a=Cod(B * Co, M, r16(M) + 48, fill=a), alo=sc(alo), ahi=sc(ahi), qlo=sc(qlo), qhi=sc(qhi)))
        host.append((a, alo, ahi, qlo, qhi))
    q1, q2, yq1, yq2, _, _, _ = ops.quant(ACT_NONE, None, r1, r2)
    z1, z2, y1, y2, _, sums, souts = ops.quant(ACT_NONE, None, r1, r2, adds=tuple(adds))
    assert torch.equal(z1, q1) and torch.equal(y1, yq1) and (not Co2 or (torch.equal(z2, q2) and torch.equal(y2, yq2)))
    dv = ops.dev
    for i, (Co, r, y) in enumerate(((Co1, r1, y1), (Co2, r2, y2))):
        if adds[i] is None:
            continue
        ad, (a, alo, ahi, qlo, qhi) = adds[i], host[i]
        yd, rs = (dv["y1"], dv["rs"][:2]) if i == 0 else (dv["y2"], dv["rs"][2:])
        ew = Cod(B * Co, M, r16(M) + 16)
        call("fqss_ewq_fwd", ad["a"].ptr, ad["alo"].ptr, ad["ahi"].ptr, yd.ptr, rs[0].ptr, rs[1].ptr, None, 1.0, ew.ptr, None, B * Co, M,
             ad["a"].ld, yd.ld, 0, ew.ld, 0, ACT_NONE, None, ad["qlo"].ptr, ad["qhi"].ptr, stream())
        assert torch.equal(sums[i], ew.cpu(B, Co, M)), (case, i)
        # float64 evaluation on the fp32 steps, and torch fp32 with the device's operation order
        da, dy, dq = delta32(alo, ahi), delta32(*r), delta32(qlo, qhi)
        z64 = (da.double() * a.double() + f32(alo).double()) + (dy.double() * y.double() + f32(r[0]).double())
        c64 = torch.clip(torch.round((z64 - f32(qlo).double()) / dq.double()), 0, 255)
        z32 = (da * a.float() + f32(alo)) + (dy * y.float() + f32(r[0]))
        c32 = torch.clip(torch.round((z32 - f32(qlo)) / dq), 0, 255)
        for name, got in (("torch fp32", c32.double()), ("kernel", sums[i].double())):
            d = (got - c64).abs()
            share = float((d > 0).double().mean())
            print(f"MEAS fwdq_add {name}: {int((d > 0).sum())} of {d.numel()} codes one level off | {case} output {i + 1}")
            assert float(d.max()) <= 1 and share <= ADD_SHARE, (case, name, share)
        assert int(sums[i].min()) == 0 and int(sums[i].max()) == 255
        cdrop = torch.clip(torch.round(((dy.double() * y.double() + f32(r[0]).double()) - f32(qlo).double()) / dq.double()), 0, 255)
        assert float(((cdrop - c64).abs() > 1).double().mean()) > 10 * ADD_SHARE, "the addend dropped"


@gpu
def test_forward_refusals():
    """each FQSS_REQUIRE of qpw_fwd_impl that the flat entries reach, the stats1 check added with this file among them; no output is
    touched"""
    B, Ci, Co1, Co2, M = 1, 32, 32, 32, 70
    g = gen(5)
    wi, c = wcodes(g, 64, 32), codes(g, B, 32, M)
    xc, wiC = Cod(B * 528, M, 96, fill=torch.zeros(B * 528, M, dtype=torch.uint8)), Cod(64, 528, fill=torch.zeros(64, 528, dtype=torch.int8))
    xo, wo = Cod(B * Ci, M, 96, off=8, fill=c), Cod(64, Ci, off=4, fill=wi)
    dw, rw, b1, b2, lo, hi = Vec(64, fill=1.0), Vec(64, fill=0.0), Vec(32, fill=0.0), Vec(32, fill=0.0), sc(0.0), sc(255.0)
    z1, z2, zo = Blk(B * 64, M, 72), Blk(B * 32, M, 76), Blk(B * 64, M, 72, off=1)
    y1, y2, yo = Cod(B * 64, M, 80), Cod(B * 32, M, 96), Cod(B * 64, M, 80, off=4)
    r = [sc(-1.0), sc(1.0), sc(-2.0), sc(2.0)]
    sl, st = sc(0.2), Slots(64)
    S = stream()

    def fwd(xc=xc.ptr, wi=wiC.ptr, dw=dw.ptr, rw=rw.ptr, b=b1.ptr, lo=lo.ptr, hi=hi.ptr, z=z1.ptr, B=B, Ci=Ci, Co=64, M=M, ldx=96, ldz=72):
        refused("fqss_qpw_fwd", xc, wi, dw, rw, b, lo, hi, z, B, Ci, Co, M, ldx, ldz, S, who="qpw_fwd")

    def fwd2(b1_=b1.ptr, b2_=b2.ptr, z2_=z2.ptr, Co2=Co2, ldz2=76, z1_=z1.ptr, who="qpw_fwd"):
        refused("fqss_qpw_fwd2", xc.ptr, wiC.ptr, dw.ptr, rw.ptr, b1_, b2_, lo.ptr, hi.ptr, z1_, z2_, B, Ci, Co1, Co2, M, 96, 72, ldz2, S, who=who)

    def fwdq(act=ACT_NONE, slope=None, Co1=32, Co2=32, q=None, yc1=y1.ptr, yc2=y2.ptr, ld1=80, ld2=96, stats=None, M=M, xcp=xc.ptr, ldx=96,
             z2_=z2.ptr, y1ld=None):
        q = [v.ptr for v in r] if q is None else q
        refused("fqss_qpw_fwdq", xcp, wiC.ptr, dw.ptr, rw.ptr, b1.ptr, b2.ptr if Co2 else None, lo.ptr, hi.ptr, z1.ptr, z2_ if Co2 else None, act,
                slope, *q, yc1, yc2 if Co2 else None, B, Ci, Co1, Co2, M, ldx, 72, 76 if Co2 else 0, ld1, ld2 if Co2 else 0, stats, S, who="qpw_fwd")

    for k in ("xc", "wi", "dw", "rw", "lo", "hi", "z"):                                   # null tensor
        fwd(**{k: None})
    fwd(ldx=64)                                                                           # bad shape: ld_xc < M
    fwd(ldz=68)
    fwd(Ci=0)
    fwd(Co=0)
    fwd(Ci=24)                                                                            # Ci % 16
    fwd(Ci=528)                                                                           # Ci > 512
    fwd(ldx=88)                                                                           # ld_xc % 16
    fwd(xc=xo.ptr)                                                                        # misaligned bases
    fwd(wi=wo.ptr)
    fwd(ldz=71)                                                                           # ld_z % 4
    fwd(z=zo.ptr)
    fwd2(z2_=None)
    fwd2(ldz2=64)
    fwd2(ldz2=78)
    fwd2(b2_=None)                                                                        # one bias of a pair missing
    fwd2(b1_=None)
    fwd2(Co2=0)                                                                           # second layer missing
    fwdq(Co1=16, Co2=48)                                                                  # fused pair with Co1 % 32 != 0
    fwdq(stats=st.ptr)                                                                    # statistics with a pair
    fwdq(act=ACT_PRELU)                                                                   # PReLU without a slope
    for k in range(4):                                                                    # fused quantizer: null pointers
        q = [v.ptr for v in r]
        q[k] = None
        fwdq(q=q)
    fwdq(yc1=None)
    fwdq(yc2=None)
    fwdq(ld1=72)                                                                          # output code rows: ld % 16, ld < M, base
    fwdq(ld2=64)
    fwdq(yc1=yo.ptr)
    # statistics for a shape without slots: Co1 = 1, M = 65 600 is 1025 tiles (the buffers are real: a launch would stay inside them)
    Mb = 65600
    assert _lib.query("fqss_qpw_stat_slots", 1, Mb) == 0 and _lib.query("fqss_qpw_stat_slots", 1, Mb - 64) == 1024
    xb, zb, yb, sb = Cod(16, Mb, Mb, fill=torch.zeros(16, Mb, dtype=torch.uint8)), Blk(1, Mb, Mb), Cod(1, Mb, Mb), Slots(2 * 1025)
    refused("fqss_qpw_fwdq", xb.ptr, wiC.ptr, dw.ptr, rw.ptr, b1.ptr, None, lo.ptr, hi.ptr, zb.ptr, None, ACT_NONE, None, r[0].ptr, r[1].ptr,
            None, None, yb.ptr, None, 1, 16, 1, 0, Mb, Mb, Mb, 0, Mb, 0, sb.ptr, S, who="qpw_fwd")
    assert zb.untouched() and yb.untouched() and sb.untouched()
    # fused AddQ
    a, ao, ys = Cod(B * 32, M, 80, fill=codes(g, B * 32, M)), Cod(B * 32, M, 80, off=4, fill=codes(g, B * 32, M)), Cod(B * 32, M, 96)

    def fwda(Co2=32, first=True, **over):
        s = _lib.FqssAddAfter()
        f = dict(a=a.ptr, ld_a=80, amin=r[0].ptr, amax=r[1].ptr, qmin=r[2].ptr, qmax=r[3].ptr, y=ys.ptr, ld_y=96)
        f.update(over)
        for k, v in f.items():
            setattr(s, k, v)
        ad = (ctypes.addressof(s), None) if first else (None, ctypes.addressof(s))
        refused("fqss_qpw_fwdq_add", xc.ptr, wiC.ptr, dw.ptr, rw.ptr, b1.ptr, b2.ptr if Co2 else None, lo.ptr, hi.ptr, z1.ptr, z2.ptr if Co2 else None,
                *[v.ptr for v in r[:2]], *([v.ptr for v in r[2:]] if Co2 else [None, None]), y1.ptr, y2.ptr if Co2 else None, B, Ci, 32, Co2, M, 96, 72,
                76 if Co2 else 0, 80, 96 if Co2 else 0, *ad, S, who="qpw_fwd")

    fwda(Co2=0, first=False)                                                              # behind a second output that does not exist
    for k in ("a", "y", "amin", "amax", "qmin", "qmax"):
        fwda(**{k: None})
    fwda(ld_a=72)
    fwda(ld_a=64)
    fwda(ld_y=88)
    fwda(a=ao.ptr)
    for o in (z1, z2, zo, y1, y2, yo, ys):
        assert o.untouched()
    assert st.untouched()
    # an empty batch is a no-op
    call("fqss_qpw_fwd", xc.ptr, wiC.ptr, dw.ptr, rw.ptr, b1.ptr, lo.ptr, hi.ptr, z1.ptr, 0, Ci, 64, M, 96, 72, S)
    assert z1.untouched()


# =============================================================================================================== 3. data gradient
# (B, Ci, Co1, Co2, M, addend).  Co > 1024 runs in parts: 1040 = 528 + 512, 1536 = 2 x 768, 2064 = 3 x 688
DG_CASES = [(1, 1, 16, 0, 1, False), (3, 16, 48, 0, 3, True), (1, 130, 512, 0, 63, False), (1, 512, 1024, 0, 64, True),
            (3, 130, 1040, 0, 65, False), (1, 16, 1536, 0, 130, True), (1, 130, 2064, 0, 65, False), (3, 16, 48, 16, 63, False),
            (1, 130, 32, 48, 130, False), (1, 512, 512, 512, 3, False), (3, 1, 1040, 0, 130, True)]


def dg_run(B, Ci, Co1, Co2, M, wi, dw, gz, addend=None):
    """fqss_qpw_bwd_x / _add / _x2 on guarded buffers (gx starts NaN-filled) -> gx on the CPU"""
    Co = Co1 + Co2
    g1 = Blk(B * Co1, M, pad4(M), fill=gz[:, :Co1])
    g2 = Blk(B * Co2, M, r4(M) + 8, fill=gz[:, Co1:]) if Co2 else None
    wT, dwv = Cod(Ci, Co, fill=wi.t()), Vec(Co, fill=dw)
    gx = Blk(B * Ci, M, r4(M) + 12)
    ops = dict(g1=g1, wT=wT, dw=dwv)
    if Co2:
        ops["g2"] = g2
        call("fqss_qpw_bwd_x2", g1.ptr, g2.ptr, wT.ptr, dwv.ptr, gx.ptr, B, Ci, Co1, Co2, M, g1.ld, g2.ld, gx.ld, stream())
    elif addend is not None:
        ops["add"] = Blk(B * Ci, M, r4(M), fill=addend)
        call("fqss_qpw_bwd_x_add", g1.ptr, wT.ptr, dwv.ptr, ops["add"].ptr, gx.ptr, B, Ci, Co, M, g1.ld, ops["add"].ld, gx.ld, stream())
    else:
        call("fqss_qpw_bwd_x", g1.ptr, wT.ptr, dwv.ptr, gx.ptr, B, Ci, Co, M, g1.ld, gx.ld, stream())
    all_unchanged(**ops)
    assert fwritten(gx)
    return gx.cpu(B, Ci, M)


def dg_exact_operands(B, Ci, Co, M, add, seed):
    g = gen(seed)
    wi, gz = wcodes(g, Co, Ci), ints(g, 8, B, Co, M)
    ad = ints(g, 1000, B, Ci, M) if add else None
    return wi, gz, ad


def dg_abs(wi, gz, ad=None):
    a = torch.einsum("oc,bom->bcm", wi.double().abs(), gz.double().abs())
    return a + ad.double().abs() if ad is not None else a


@gpu
@pytest.mark.parametrize("case", DG_CASES, ids=str)
def test_dgrad_exact_integers(case):
    """dw = 1, integer gz (|gz| <= 8) and addend: gx is the integer sum bit for bit, through every part of a Co > 1024 reduction"""
    B, Ci, Co1, Co2, M, add = case
    Co = Co1 + Co2
    wi, gz, ad = dg_exact_operands(B, Ci, Co, M, add, 500 + Ci + Co + M)
    assert exact_ok(dg_abs(wi, gz, ad))
    gx = dg_run(B, Ci, Co1, Co2, M, wi, torch.ones(Co), gz, ad)
    assert torch.equal(gx, dgrad_ref(wi, torch.ones(Co), gz, ad).float()), case
    differs(dgrad_ref(wi.roll(1, 0), torch.ones(Co), gz, ad), dgrad_ref(wi, torch.ones(Co), gz, ad), "reduction row one off", f"dgrad exact {case}")


def pieces_operands(kind, seed):
    """gz = n 2^-20 whose split reaches the second ("two": |n| < 2^10, full int8 weight codes, K <= 64) or the third bf16 piece
    ("three": |n| < 2^17, 4-bit weight codes [-8, 7], K = 16)"""
    g = gen(seed)
    if kind == "two":
        B, Ci, Co, M = 2, 33, 64, 65
        wi = wcodes(g, Co, Ci)
        n = torch.randint(-1023, 1024, (B, Co, M), generator=g)
    else:
        B, Ci, Co, M = 2, 130, 16, 63
        wi = wcodes(g, Co, Ci, lim=8)
        n = torch.randint(-(2 ** 17) + 1, 2 ** 17, (B, Co, M), generator=g)
    return B, Ci, Co, M, wi, n.float() * 2.0 ** -20, n


@gpu
@pytest.mark.parametrize("kind", ["two", "three"])
def test_dgrad_exact_through_the_bf16_pieces(kind):
    """gz = n 2^-s with more than 8 (16) significant bits: the second (third) bf16 piece carries part of every product and every partial
    sum stays an exact multiple of 2^-s below 2^24: bit-equal.  The 4-bit weight codes come from fqss_wq_codes_bits"""
    B, Ci, Co, M, wi, gz, n = pieces_operands(kind, 7)
    h1, h2, h3 = split3(gz)
    assert bool((h2 != 0).any()) and (kind == "two" or bool((h3 != 0).any()))
    assert exact_ok(dg_abs(wi, n))
    if kind == "three":
        idx, idxT, dwk, _ = wq_run(wi.float(), torch.full((Co,), -7.5), torch.full((Co,), 7.5), 4)
        assert torch.equal(idx, wi) and torch.equal(dwk, torch.ones(Co))
    ref = dgrad_ref(wi, torch.ones(Co), gz)
    gx = dg_run(B, Ci, Co, 0, M, wi, torch.ones(Co), gz)
    assert torch.equal(gx, ref.float()), kind
    differs(dgrad_ref(wi, torch.ones(Co), h1 + h2 if kind == "three" else h1), ref, f"bf16 piece {3 if kind == 'three' else 2} of gz dropped",
            f"dgrad pieces {kind}")


def dg_real_operands(B, Ci, Co, M, add, seed):
    g = gen(seed)
    wi, dw, gz = wcodes(g, Co, Ci), steps(g, Co), heavy(g, B, Co, M)
    ad = torch.randn(B, Ci, M, generator=g) * 1e-3 if add else None
    return wi, dw, gz, ad


@gpu
@pytest.mark.parametrize("case", DG_CASES, ids=str)
def test_dgrad_against_fp64(case):
    """heavy-tailed gz, real steps: fqss_qpw_bwd_x / _add / _x2 against float64 and the mutation floors of the family"""
    B, Ci, Co1, Co2, M, add = case
    Co = Co1 + Co2
    wi, dw, gz, ad = dg_real_operands(B, Ci, Co, M, add, 600 + Ci + Co + M)
    gx = dg_run(B, Ci, Co1, Co2, M, wi, dw, gz, ad)
    ref = dgrad_ref(wi, dw, gz, ad)
    w32 = wi.float() * dw[:, None]
    r32 = torch.einsum("oc,bom->bcm", w32, gz) + (ad if add else 0.0)
    fails, tag = [], f"dgrad {case}"
    measure("dgrad", "gx", gx, ref, r32, tag, fails)
    assert not fails, fails
    kl = (Co - 1) // 32 * 32
    if kl > 0:
        floor("dgrad", "gx", dgrad_ref(wi[:kl], dw[:kl], gz[:, :kl], ad), ref, "last k-tile dropped", tag)
    floor("dgrad", "gx", dgrad_ref(wi, dw.roll(1), gz, ad), ref, "dw of the neighbouring row", tag)
    if Co2:
        g2 = torch.cat([gz[:, :Co1], gz[:, Co1:].roll(1, 1)], 1)
        floor("dgrad", "gx", dgrad_ref(wi, dw, g2, ad), ref, "pair split one row off", tag)
    if add:
        floor("dgrad", "gx", dgrad_ref(wi, dw, gz), ref, "the addend dropped", tag)
    if Co > 1024:
        part = (-(-Co // -(-Co // 1024)) + 15) // 16 * 16
        keep = torch.ones(Co, dtype=torch.bool)
        keep[part:2 * part] = False
        floor("dgrad", "gx", dgrad_ref(wi[keep], dw[keep], gz[:, keep], ad), ref, "second part of the reduction dropped", tag)
    h1, h2, _ = split3(gz * dw[None, :, None])
    fl = errs(torch.einsum("oc,bom->bcm", wi.double(), (h1 + h2).double()) + (ad.double() if add else 0.0), ref)
    print(f"FLOOR dgrad gx third bf16 piece dropped {fl[0]:.2e} / {fl[1]:.2e} (bound {BOUND['dgrad']['gx']}; void here, see the docstring) | {tag}")


@gpu
def test_dgrad_in_parts_equals_two_launches():
    """Co = 1536 = 2 x 768: part 1 adds to what part 0 left in gx, an fp32 add per element -- bit-equal to two single launches on the
    halves (their own dense W^T) summed on the host; the addend travels with part 0"""
    B, Ci, Co, M = 1, 130, 1536, 65
    wi, dw, gz, ad = dg_real_operands(B, Ci, Co, M, True, 77)
    for addend in (None, ad):
        whole = dg_run(B, Ci, Co, 0, M, wi, dw, gz, addend)
        a = dg_run(B, Ci, 768, 0, M, wi[:768], dw[:768], gz[:, :768], addend)
        b = dg_run(B, Ci, 768, 0, M, wi[768:], dw[768:], gz[:, 768:])
        assert torch.equal(whole, a + b)


@gpu
def test_dgrad_refusals():
    B, Ci, Co, M = 1, 16, 32, 70
    g = gen(9)
    wT, wo, dw = Cod(Ci, 1040, fill=torch.zeros(Ci, 1040, dtype=torch.int8)), Cod(Ci, Co, off=4, fill=wcodes(g, Ci, Co)), Vec(1040, fill=1.0)
    gz, go, ad, ao = [Blk(B * 1040, M, 72, off=o, fill=torch.zeros(B * 1040, M)) for o in (0, 1)] + [Blk(B * Ci, M, 72, off=o, fill=torch.zeros(B * Ci, M))
                                                                                                    for o in (0, 2)]
    gx, gxo = Blk(B * Ci, M, 76), Blk(B * Ci, M, 76, off=3)
    S = stream()

    def bx(gz_=gz.ptr, wT_=wT.ptr, dw_=dw.ptr, gx_=gx.ptr, B=B, Ci=Ci, Co=Co, M=M, ldg=72, ldx=76):
        refused("fqss_qpw_bwd_x", gz_, wT_, dw_, gx_, B, Ci, Co, M, ldg, ldx, S, who="qpw_bwd_x")

    def bxa(ad_=ad.ptr, lda=72):
        refused("fqss_qpw_bwd_x_add", gz.ptr, wT.ptr, dw.ptr, ad_, gx.ptr, B, Ci, Co, M, 72, lda, 76, S, who="qpw_bwd_x")

    def bx2(g2=gz.ptr, Co1=16, Co2=16, ld2=72):
        refused("fqss_qpw_bwd_x2", gz.ptr, g2, wT.ptr, dw.ptr, gx.ptr, B, Ci, Co1, Co2, M, 72, ld2, 76, S, who="qpw_bwd_x")

    for k in ("gz_", "wT_", "dw_", "gx_"):
        bx(**{k: None})
    bx(ldg=68)                           # bad shape
    bx(ldx=68)
    bx(Ci=0)
    bx(Co=24)                            # Co % 16
    bx(ldg=74)                           # ld_gz % 4
    bx(gz_=go.ptr)
    bx(wT_=wo.ptr)
    bx(ldx=78)                           # output rows
    bx(gx_=gxo.ptr)
    bxa(ad_=None)
    bxa(ad_=ao.ptr)
    bxa(lda=74)
    bxa(lda=68)
    bx2(g2=None)
    bx2(Co2=0)
    bx2(Co2=24)
    bx2(ld2=74)
    bx2(g2=go.ptr)
    bx2(Co1=528, Co2=512)                # a pair stays at Co1 + Co2 <= 1024
    assert gx.untouched() and gxo.untouched()
    call("fqss_qpw_bwd_x", gz.ptr, wT.ptr, dw.ptr, gx.ptr, B, Ci, Co, 0, 72, 76, S)
    assert gx.untouched()


# ============================================================================================================= 4. weight gradient
# (B, Ci, Co1, Co2, M).  (1, 128, 64, 0, 257) is ONE 64 x 128 tile: kchunk = 256 and a second split of one column
WG_CASES = [(1, 16, 1, 0, 1), (3, 128, 64, 0, 3), (1, 130, 65, 0, 63), (1, 256, 200, 0, 64), (3, 300, 1, 0, 65), (1, 16, 64, 0, 255),
            (1, 128, 64, 0, 257), (1, 130, 200, 0, 256), (3, 300, 64, 0, 1030), (3, 16, 48, 16, 257), (1, 256, 128, 128, 65),
            (1, 130, 144, 40, 1030)]


class WgOps:
    def __init__(self, B, Ci, Co1, Co2, M, gz, c, lo, hi, k=0):
        self.dims = (B, Ci, Co1, Co2, M)
        self.g1 = Blk(B * Co1, M, pad4(M, 4 + 4 * (k % 2)), fill=gz[:, :Co1])
        self.g2 = Blk(B * Co2, M, r4(M) + 16, fill=gz[:, Co1:]) if Co2 else None
        self.xc = Cod(B * Ci, M, r16(M) + 32, fill=c)
        self.lo, self.hi = sc(lo), sc(hi)

    def unchanged(self):
        ops = dict(g1=self.g1, xc=self.xc, lo=self.lo, hi=self.hi)
        if self.g2 is not None:
            ops["g2"] = self.g2
        all_unchanged(**ops)

    def single(self, start, gw_ptr=None):
        """fqss_qpw_bwd_w / _w2 into a guarded gw that starts at `start` -> gw on the CPU"""
        B, Ci, Co1, Co2, M = self.dims
        gw = Vec((Co1 + Co2) * Ci, fill=start) if gw_ptr is None else None
        p = gw.ptr if gw_ptr is None else gw_ptr
        if Co2:
            call("fqss_qpw_bwd_w2", self.g1.ptr, self.g2.ptr, self.xc.ptr, self.lo.ptr, self.hi.ptr, p, B, Ci, Co1, Co2, M, self.g1.ld, self.g2.ld,
                 self.xc.ld, stream())
        else:
            call("fqss_qpw_bwd_w", self.g1.ptr, self.xc.ptr, self.lo.ptr, self.hi.ptr, p, B, Ci, Co1, M, self.g1.ld, self.xc.ld, stream())
        self.unchanged()
        if gw is None:
            return None
        assert gw.written()
        return gw.cpu(Co1 + Co2, Ci)

    def job(self, j, gw):
        B, Ci, Co1, Co2, M = self.dims
        j.gz1, j.gz2, j.xc, j.qmin_x, j.qmax_x, j.gw = self.g1.ptr, (self.g2.ptr if Co2 else None), self.xc.ptr, self.lo.ptr, self.hi.ptr, gw.ptr
        j.B, j.Ci, j.Co1, j.Co2, j.M = B, Ci, Co1, Co2, M
        j.ld_gz1, j.ld_gz2, j.ld_xc = self.g1.ld, (self.g2.ld if Co2 else 0), self.xc.ld


class Work:
    """the workspace of fqss_qpw_bwd_w_group: `need` zero bytes between SENT guard bytes"""

    def __init__(self, need):
        self.need = need
        self.buf = torch.full((need + 2 * GB,), SENT, dtype=torch.uint8, device=DEV)
        self.buf[GB:GB + need] = 0
        self.ptr = self.buf.data_ptr() + GB

    def clean(self):
        """guards untouched, the 64 KB of arrival tickets all zero"""
        return bool((self.buf[:GB] == SENT).all()) and bool((self.buf[GB + self.need:] == SENT).all()) and bool((self.buf[GB:GB + 65536] == 0).all())


def group_run(opss, starts):
    """one fqss_qpw_bwd_w_group call over the jobs, workspace from _ws -> the gw's on the CPU"""
    n = len(opss)
    arr = (_lib.FqssWgradJob * n)()
    gws = [Vec((o.dims[2] + o.dims[3]) * o.dims[1], fill=s) for o, s in zip(opss, starts)]
    for j, o, gw in zip(arr, opss, gws):
        o.job(j, gw)
    need = _lib.query("fqss_qpw_bwd_w_group_ws", arr, n)
    assert need >= 65536
    ws = Work(need)
    call("fqss_qpw_bwd_w_group", arr, n, ws.ptr, need, stream())
    assert ws.clean()
    for o, gw in zip(opss, gws):
        o.unchanged()
        assert gw.written()
    return [gw.cpu(o.dims[2] + o.dims[3], o.dims[1]) for o, gw in zip(opss, gws)], (arr, ws, gws)


def wg_exact_operands(B, Ci, Co, M, seed):
    g = gen(seed)
    return ints(g, 8, B, Co, M), codes(g, B, Ci, M), ints(g, 1000, Co, Ci)


@gpu
@pytest.mark.parametrize("case", WG_CASES, ids=str)
def test_wgrad_exact_integers(case):
    """|gz| <= 8 integers, dx = 1, min_x = 0, an integer start in gw: fqss_qpw_bwd_w / _w2 and fqss_qpw_bwd_w_group give the integer sum
    bit for bit, whatever order the atomics arrive in"""
    B, Ci, Co1, Co2, M = case
    Co = Co1 + Co2
    gz, c, start = wg_exact_operands(B, Ci, Co, M, 700 + Ci + Co + M)
    assert B * M * 8 * 255 + 1000 < TWO24 and exact_ok(torch.einsum("bom,bcm->oc", gz.double().abs(), c.double()) + start.abs())
    ops = WgOps(B, Ci, Co1, Co2, M, gz, c, 0.0, 255.0, k=M)
    ref = (start.double() + wgrad_ref(gz, c, 0.0, 255.0)).float()
    assert torch.equal(ops.single(start), ref), case
    assert torch.equal(group_run([ops], [start])[0][0], ref), case
    tag = f"wgrad exact {case}"
    if M > 1:
        differs(wgrad_ref(gz[..., :M - 1], c[..., :M - 1], 0.0, 255.0), wgrad_ref(gz, c, 0.0, 255.0), "last live column dropped", tag)
    if B > 1:
        differs(wgrad_ref(gz[:B - 1], c[:B - 1], 0.0, 255.0), wgrad_ref(gz, c, 0.0, 255.0), "last batch dropped", tag)


@gpu
def test_wgrad_exact_integers_with_offset():
    """an integer min_x = -3 (range [-3, 252]: dx = 1): the row-sum term, exact in all three entries"""
    for k, (B, Ci, Co1, Co2, M) in enumerate([(3, 130, 65, 0, 257), (1, 300, 48, 16, 1030), (1, 16, 1, 0, 3)]):
        gz, c, start = wg_exact_operands(B, Ci, Co1 + Co2, M, 750 + k)
        assert exact_ok(torch.einsum("bom,bcm->oc", gz.double().abs(), c.double() + 3) + start.abs())
        ops = WgOps(B, Ci, Co1, Co2, M, gz, c, -3.0, 252.0, k=k)
        ref = (start.double() + wgrad_ref(gz, c, -3.0, 252.0)).float()
        assert torch.equal(ops.single(start), ref)
        assert torch.equal(group_run([ops], [start])[0][0], ref)
        differs(start.double() + wgrad_ref(gz, c, -3.0, 252.0, dropmin=True), ref, "min_x rowsum dropped", f"wgrad offset {k}")


@gpu
def test_wgrad_exact_through_the_bf16_pieces():
    """gz = n 2^-20 with |n| < 2^17 (17 significant bits: all three bf16 pieces) against codes 0 .. 3 at M = 33: every partial sum is an
    exact multiple of 2^-20 below 2^24 of them, so all three entries are bit-equal -- and a kernel without the third piece is not"""
    B, Ci, Co1, Co2, M = 1, 130, 49, 16, 33
    g = gen(17)
    n = torch.randint(-(2 ** 17) + 1, 2 ** 17, (B, Co1 + Co2, M), generator=g)
    gz, c = n.float() * 2.0 ** -20, torch.randint(0, 4, (B, Ci, M), generator=g, dtype=torch.uint8)
    start = ints(g, 1000, Co1 + Co2, Ci) * 2.0 ** -20
    h1, h2, h3 = split3(gz)
    assert bool((h3 != 0).any()) and exact_ok(torch.einsum("bom,bcm->oc", n.double().abs(), c.double()) + 1000)
    ref = start.double() + wgrad_ref(gz, c, 0.0, 255.0)
    for Ca, Cb in ((Co1, Co2), (Co1 + Co2, 0)):
        ops = WgOps(B, Ci, Ca, Cb, M, gz, c, 0.0, 255.0)
        assert torch.equal(ops.single(start), ref.float())
        assert torch.equal(group_run([ops], [start])[0][0], ref.float())
    differs(start.double() + wgrad_ref(h1 + h2, c, 0.0, 255.0), ref, "bf16 piece 3 of gz dropped", "wgrad pieces")
    differs(start.double() + wgrad_ref(h1, c, 0.0, 255.0), start.double() + wgrad_ref(h1 + h2, c, 0.0, 255.0), "bf16 piece 2 of gz dropped", "wgrad pieces")


def wg_real_operands(B, Ci, Co, M, seed):
    g = gen(seed)
    gz, c = heavy(g, B, Co, M), codes(g, B, Ci, M)
    return gz, c, -1.3, 2.1


def wg_floors(fam, gz, c, lo, hi, ref, case, tag):
    B, Ci, Co1, Co2, M = case
    ml = (M - 1) // 64 * 64
    if ml > 0:
        floor(fam, "gw", wgrad_ref(gz[..., :ml], c[..., :ml], lo, hi), ref, "last 64-column stage dropped", tag)
    floor(fam, "gw", wgrad_ref(gz, c, lo, hi, dropmin=True), ref, "min_x rowsum dropped", tag)
    if Co2:
        g2 = torch.cat([gz[:, :Co1], gz[:, Co1:].roll(1, 1)], 1)
        floor(fam, "gw", wgrad_ref(g2, c, lo, hi), ref, "pair split one row off", tag)
    if M > 1:
        floor(fam, "gw", wgrad_ref(gz[..., :M - 1], c[..., :M - 1], lo, hi), ref, "last live column dropped", tag)
    one, c255 = torch.full_like(gz[..., :1], rms(gz)), torch.full_like(c[..., :1], 255)
    floor(fam, "gw", wgrad_ref(torch.cat([gz, one], 2), torch.cat([c, c255], 2), lo, hi), ref, "padding column M read (gz of the rms, code 255)", tag)
    if B > 1:
        floor(fam, "gw", wgrad_ref(gz[:B - 1], c[:B - 1], lo, hi), ref, "last batch dropped", tag)
    h1, h2, _ = split3(gz)
    fl = errs(wgrad_ref(h1 + h2, c, lo, hi), ref)
    print(f"FLOOR {fam} gw third bf16 piece dropped {fl[0]:.2e} / {fl[1]:.2e} (bound {BOUND[fam]['gw']}; void here, see the docstring) | {tag}")


@gpu
@pytest.mark.parametrize("case", WG_CASES, ids=str)
def test_wgrad_against_fp64(case):
    """heavy-tailed gz, range [-1.3, 2.1], gw accumulated into a non-zero start: the per-layer kernel (fp32 atomics) and the grouped one
    (slab slots in part order) against float64, and the mutation floors"""
    B, Ci, Co1, Co2, M = case
    Co = Co1 + Co2
    gz, c, lo, hi = wg_real_operands(B, Ci, Co, M, 800 + Ci + Co + M)
    ref = wgrad_ref(gz, c, lo, hi)
    start = torch.randn(Co, Ci, generator=gen(1)) * rms(ref)
    x32 = delta32(lo, hi) * c.float() + f32(lo)
    r32 = torch.einsum("bom,bcm->oc", gz, x32)
    ops = WgOps(B, Ci, Co1, Co2, M, gz, c, lo, hi, k=M)
    fails, tag = [], f"wgrad {case}"
    measure("wgrad", "gw", ops.single(start).double() - start.double(), ref, r32, tag, fails)
    measure("group", "gw", group_run([ops], [start])[0][0].double() - start.double(), ref, r32, tag, fails)
    assert not fails, fails
    wg_floors("wgrad", gz, c, lo, hi, ref, case, tag)
    wg_floors("group", gz, c, lo, hi, ref, case, tag)


@gpu
def test_wgrad_group_many_jobs():
    """26 small jobs (two launches of 13), one of them smaller than a tile, pairs and the wide tile among them: against float64, the
    tickets zero afterwards, two runs bit-identical; shared gw and a short workspace are refused"""
    shapes = [(1 + k % 3, (16, 130, 256, 48)[k % 4], (1, 64, 65, 48)[k % 4], (0, 0, 0, 16)[k % 4], (3, 63, 65, 257, 130)[k % 5]) for k in range(26)]
    shapes[5] = (1, 16, 3, 0, 5)                                   # smaller than one tile in every direction
    opss, starts, refs = [], [], []
    for k, (B, Ci, Co1, Co2, M) in enumerate(shapes):
        gz, c, lo, hi = wg_real_operands(B, Ci, Co1 + Co2, M, 900 + k)
        refs.append(wgrad_ref(gz, c, lo, hi))
        starts.append(torch.randn(Co1 + Co2, Ci, generator=gen(k)) * rms(refs[-1]))
        opss.append(WgOps(B, Ci, Co1, Co2, M, gz, c, lo, hi, k=k))
    run1, (arr, ws, gws) = group_run(opss, starts)
    run2, _ = group_run(opss, starts)
    fails = []
    for k, (a, b, ref, st) in enumerate(zip(run1, run2, refs, starts)):
        assert torch.equal(a, b), (k, "not reproducible")
        measure("group", "gw", a.double() - st.double(), ref, None, f"group job {k} {shapes[k]}", fails)
    assert not fails, fails
    n = len(opss)
    before = [gw.buf.clone() for gw in gws]
    one = (_lib.FqssWgradJob * 1)()
    opss[3].job(one[0], gws[3])
    need1 = _lib.query("fqss_qpw_bwd_w_group_ws", one, 1)
    assert 65536 < need1 <= ws.need
    refused("fqss_qpw_bwd_w_group", one, 1, ws.ptr, need1 - 1, stream())                           # a workspace one byte short
    refused("fqss_qpw_bwd_w_group", arr, n, ws.ptr + 4, ws.need, stream())
    refused("fqss_qpw_bwd_w_group", arr, n, None, ws.need, stream())
    two = (_lib.FqssWgradJob * 2)()
    opss[0].job(two[0], gws[0])
    opss[0].job(two[1], gws[0])                                                                    # two jobs sharing gw
    refused("fqss_qpw_bwd_w_group", two, 2, ws.ptr, ws.need, stream(), who="wgr_check")
    assert _lib.query("fqss_qpw_bwd_w_group_ws", two, 2) == -1 and _lib.query("fqss_qpw_bwd_w_group_ws", arr, 0) == -1
    assert all(torch.equal(L._bits(gw.buf), L._bits(b)) for gw, b in zip(gws, before)) and ws.clean()


@gpu
def test_wgrad_refusals():
    B, Ci, Co, M = 1, 16, 32, 70
    gz, go = [Blk(B * Co, M, 72, off=o, fill=torch.zeros(B * Co, M)) for o in (0, 1)]
    xc, xo = [Cod(B * Ci, M, 80, off=o, fill=torch.zeros(B * Ci, M, dtype=torch.uint8)) for o in (0, 4)]
    lo, hi, gw = sc(0.0), sc(255.0), Vec(Co * Ci)
    S = stream()

    def bw(gz_=gz.ptr, xc_=xc.ptr, lo_=lo.ptr, hi_=hi.ptr, gw_=gw.ptr, Ci=Ci, Co=Co, M=M, ldg=72, ldx=80):
        refused("fqss_qpw_bwd_w", gz_, xc_, lo_, hi_, gw_, B, Ci, Co, M, ldg, ldx, S, who="qpw_bwd_w")
        j = (_lib.FqssWgradJob * 1)()
        j[0].gz1, j[0].xc, j[0].qmin_x, j[0].qmax_x, j[0].gw = gz_, xc_, lo_, hi_, gw_
        j[0].B, j[0].Ci, j[0].Co1, j[0].Co2, j[0].M, j[0].ld_gz1, j[0].ld_xc = B, Ci, Co, 0, M, ldg, ldx
        assert _lib.query("fqss_qpw_bwd_w_group_ws", j, 1) == -1
        refused("fqss_qpw_bwd_w_group", j, 1, gw.ptr, 0, S, who="wgr_check")

    def bw2(g2=gz.ptr, Co2=16, ld2=72):
        refused("fqss_qpw_bwd_w2", gz.ptr, g2, xc.ptr, lo.ptr, hi.ptr, gw.ptr, B, Ci, 16, Co2, M, 72, ld2, 80, S, who="qpw_bwd_w")

    for k in ("gz_", "xc_", "lo_", "hi_", "gw_"):
        bw(**{k: None})
    bw(ldg=68)
    bw(ldx=64)
    bw(Ci=0)
    bw(Co=0)
    bw(ldg=74)
    bw(ldx=88)
    bw(gz_=go.ptr)
    bw(xc_=xo.ptr)
    bw2(g2=None)
    bw2(Co2=0)
    bw2(ld2=74)
    bw2(g2=go.ptr)
    assert gw.untouched()


@pytest.fixture
def det_off():
    yield
    if K is not None:
        K.DetMode.off()          # (the control block is device-wide: no later test may run under it)


@gpu
def test_wgrad_deterministic_mode(det_off):
    """FQSS_DETERMINISTIC=1 arithmetic of k_qwgrad2's atomics (integer sums on the shadow of the attached slot-0 arena, fqss_det_finish
    rounds once): two runs of fqss_qpw_bwd_w into a slice of the arena are bit-identical and within the bound"""
    B, Ci, Co, M = 3, 130, 65, 1030
    gz, c, lo, hi = wg_real_operands(B, Ci, Co, M, 31)
    ref = wgrad_ref(gz, c, lo, hi)
    start = torch.randn(Co, Ci, generator=gen(2)) * rms(ref)
    ops = WgOps(B, Ci, Co, 0, M, gz, c, lo, hi)
    off, n = 64, Co * Ci
    arena = torch.zeros(n + 128, device=DEV)
    det = K.DetMode()
    det.attach(0, arena)
    det.activate()
    runs = []
    for _ in range(2):
        arena.zero_()
        arena[off:off + n].copy_(start.reshape(-1))
        ops.single(None, gw_ptr=arena.data_ptr() + 4 * off)
        det.finish(0)
        sync()
        runs.append(arena.cpu().clone())
    K.DetMode.off()
    assert torch.equal(runs[0], runs[1]), "deterministic mode: the sums of two runs differ"
    a = runs[0]
    assert bool((a[:off] == 0).all()) and bool((a[off + n:] == 0).all()), "a write beside the gradient slot"
    fails = []
    measure("wgrad", "gw", a[off:off + n].reshape(Co, Ci).double() - start.double(), ref, None, "deterministic k_qwgrad2", fails)
    assert not fails, fails


# ======================================================================================================== 5. float-operand modes
# (B, Ci, Co, M, bias); the coded-weight form needs Ci % 16 == 0
PW_CASES = [(1, 4, 1, 1, False), (3, 20, 33, 3, True), (1, 128, 130, 63, True), (3, 432, 512, 130, False), (1, 4, 512, 64, True),
            (3, 128, 33, 65, True), (1, 20, 130, 130, False), (1, 432, 1, 65, True)]
PWQ_CASES = [(1, 16, 1, 1, False), (3, 48, 33, 3, True), (1, 128, 130, 63, True), (3, 432, 512, 130, False), (1, 16, 512, 64, True),
             (3, 128, 33, 65, True), (1, 432, 130, 130, False)]


def pw_run(entry, B, Ci, Co, M, w, x, b, dw=None):
    xb = Blk(B * Ci, M, pad4(M, 8), fill=x)
    bv = Vec(Co, fill=b) if b is not None else None
    z = Blk(B * Co, M, pad4(M))
    ops = dict(x=xb)
    if bv is not None:
        ops["b"] = bv
    if dw is None:
        ops["w"] = Blk(Co, Ci, fill=w)
        call(entry, xb.ptr, ops["w"].ptr, bv.ptr if bv else None, z.ptr, B, Ci, Co, M, xb.ld, z.ld, stream())
    else:
        ops["w"], ops["dw"] = Cod(Co, Ci, fill=w), Vec(Co, fill=dw)
        call(entry, xb.ptr, ops["w"].ptr, ops["dw"].ptr, bv.ptr if bv else None, z.ptr, B, Ci, Co, M, xb.ld, z.ld, stream())
    all_unchanged(**ops)
    assert fwritten(z)
    return z.cpu(B, Co, M)


@gpu
@pytest.mark.parametrize("case", PW_CASES, ids=str)
def test_float_forward_against_fp64(case):
    """fqss_pwconv_fwd_x3 (nine products) and fqss_pwconv_fwd_x3s (six) on a NaN-padded x, K tails of 4 and 20"""
    B, Ci, Co, M, bias = case
    g = gen(1000 + Ci + Co + M)
    w, x = torch.randn(Co, Ci, generator=g) * Ci ** -0.5, torch.randn(B, Ci, M, generator=g)
    b = torch.randn(Co, generator=g) if bias else None
    ref, r32 = pw_ref(w, x, b), F.conv1d(x, w[:, :, None], b)
    fails, tag = [], f"pwconv {case}"
    for fam, entry in (("x3", "fqss_pwconv_fwd_x3"), ("x3s", "fqss_pwconv_fwd_x3s")):
        measure(fam, "z", pw_run(entry, B, Ci, Co, M, w, x, b), ref, r32, tag, fails)
        kl = (Ci - 1) // 32 * 32
        floor(fam, "z", pw_ref(w[:, :kl], x[:, :kl], b) if kl else pw_ref(w[:, :Ci - 4], x[:, :Ci - 4], b) if Ci > 4 else pw_ref(w * 0, x, b), ref,
              "last k-tile (Ci <= 32: last four k) dropped", tag)
        if bias:
            floor(fam, "z", pw_ref(w, x, None), ref, "bias dropped", tag)
    assert not fails, fails


@gpu
@pytest.mark.parametrize("case", PWQ_CASES, ids=str)
def test_coded_weight_float_forward_against_fp64(case):
    """fqss_pwconv_fwd_wq: int8 weight codes x float x in three pieces"""
    B, Ci, Co, M, bias = case
    g = gen(1100 + Ci + Co + M)
    wi, dw, x = wcodes(g, Co, Ci), steps(g, Co) * 10, torch.randn(B, Ci, M, generator=g)
    b = torch.randn(Co, generator=g) if bias else None
    w64 = wi.double() * dw.double()[:, None]
    ref, r32 = pw_ref(w64, x, b), F.conv1d(x, (wi.float() * dw[:, None])[:, :, None], b)
    fails, tag = [], f"pwconv wq {case}"
    measure("wq", "z", pw_run("fqss_pwconv_fwd_wq", B, Ci, Co, M, wi, x, b, dw=dw), ref, r32, tag, fails)
    assert not fails, fails
    kl = (Ci - 1) // 32 * 32
    if kl:
        floor("wq", "z", pw_ref(w64[:, :kl], x[:, :kl], b), ref, "last k-tile dropped", tag)
    if Co > 1:
        floor("wq", "z", pw_ref(wi.double() * dw.double().roll(1)[:, None], x, b), ref, "dw of the neighbouring row", tag)


@gpu
def test_float_forward_exact_integers_and_refusals():
    """integer operands are exact in all three entries; each FQSS_REQUIRE of the two impls"""
    B, Ci, Co, M = 3, 48, 33, 65
    g = gen(12)
    wi, x, b = wcodes(g, Co, Ci), ints(g, 200, B, Ci, M), ints(g, 1000, Co)
    assert exact_ok(torch.einsum("oc,bcm->bom", wi.double().abs(), x.double().abs()) + 1000)
    ref = pw_ref(wi, x, b).float()
    assert torch.equal(pw_run("fqss_pwconv_fwd_x3", B, Ci, Co, M, wi.float(), x, b), ref)
    assert torch.equal(pw_run("fqss_pwconv_fwd_x3s", B, Ci, Co, M, wi.float(), x, b), ref)
    assert torch.equal(pw_run("fqss_pwconv_fwd_wq", B, Ci, Co, M, wi, x, b, dw=torch.ones(Co)), ref)
    xb, xo = [Blk(B * Ci, M, 72, off=o, fill=x) for o in (0, 1)]
    wb, wo, wc, wco = Blk(Co, Ci, fill=wi.float()), Blk(Co, Ci, off=2, fill=wi.float()), Cod(Co, Ci, fill=wi), Cod(Co, Ci, off=4, fill=wi)
    dw, z, zo = Vec(Co, fill=1.0), Blk(B * Co, M, 68), Blk(B * Co, M, 68, off=3)
    S = stream()
    for entry in ("fqss_pwconv_fwd_x3", "fqss_pwconv_fwd_x3s", "fqss_pwconv_fwd_wq"):
        coded = entry.endswith("wq")

        def f(x_=xb.ptr, w_=(wc if coded else wb).ptr, z_=z.ptr, Ci=Ci, Co=Co, M=M, ldx=72, ldz=68, dw_=dw.ptr):
            mid = (dw_,) if coded else ()
            refused(entry, x_, w_, *mid, None, z_, B, Ci, Co, M, ldx, ldz, S, who="pwconv_fwd")

        for k in ("x_", "w_", "z_") + (("dw_",) if coded else ()):
            f(**{k: None})
        f(ldx=64)
        f(ldz=64)
        f(Co=0)
        f(Ci=8 if coded else 6)          # Ci % 16 (coded weight) / Ci % 4
        f(ldx=70)
        f(M=66, ldx=66)                  # ld_x >= M but below roundup4(M)
        f(x_=xo.ptr)
        f(w_=(wco if coded else wo).ptr)
        f(ldz=70)
        f(z_=zo.ptr)
    assert z.untouched() and zo.untouched()


# ==================================================================================================== the references, without a GPU
def test_references_on_cpu():
    """the float64 references of this file equal float64 F.conv1d on oracle weight_quantize / act_quantize operands and that graph's
    autograd (ranges with steps that are exact in fp32, so that the fp32 step of the references is the oracle's float64 one); the integer
    constructions stay below 2^24 in the sum of their absolute products"""
    g = gen(3)
    B, Ci, Co, M = 2, 48, 33, 65
    w = (torch.randn(Co, Ci, 1, generator=g) * 0.05).double()
    a = (127.5 * 2.0 ** -9 * (1 + torch.arange(Co) % 3)).double()[:, None, None]
    xlo, xhi = torch.tensor([-0.75], dtype=F64), torch.tensor([-0.75 + 255 * 2.0 ** -7], dtype=F64)
    x = (torch.randn(B, Ci, M, generator=g) * 0.8 + 0.4).double()
    b = torch.randn(Co, generator=g).double()
    wi, c = O.weight_indices(w, -a, a)[:, :, 0], O.act_indices(x, xlo, xhi)
    dw = (2 * a / 255)[:, 0, 0].float()
    assert torch.equal(dw.double(), (2 * a / 255)[:, 0, 0]) and float(delta32(float(xlo), float(xhi))) == 2.0 ** -7
    wq = O.weight_quantize(w, -a, a).requires_grad_()
    xq = O.act_quantize(x, xlo, xhi).requires_grad_()
    z = F.conv1d(xq, wq, b)
    ref = fwd_ref(wi, c, dw, b.float().double(), float(xlo), float(xhi))
    assert errs(F.conv1d(xq, wq, b.float().double()).detach(), ref)[0] <= 1e-12
    gz = heavy(g, B, Co, M)
    z.backward(gz.double())
    assert errs(xq.grad, dgrad_ref(wi, dw, gz))[0] <= 1e-12
    assert errs(wq.grad[:, :, 0], wgrad_ref(gz, c, float(xlo), float(xhi)))[0] <= 1e-12
    assert errs(pw_ref(wq.detach()[:, :, 0], x, b), F.conv1d(x, wq.detach(), b))[0] <= 1e-12
    # split3 is exact, and the second / third pieces of the piece cases are there
    h1, h2, h3 = split3(gz)
    assert torch.equal((h1.double() + h2.double() + h3.double()).float(), gz) and bool((h3 != 0).any())
    for kind in ("two", "three"):
        _, _, Cok, _, wik, gzk, n = pieces_operands(kind, 7)
        p1, p2, p3 = split3(gzk)
        assert exact_ok(dg_abs(wik, n)) and bool((p2 != 0).any()) and (kind == "two" or bool((p3 != 0).any()))
        assert torch.equal(p1 + p2 + p3, gzk) and (kind == "three" or bool((p3 == 0).all()))
    # the exact-integer constructions: sum |products| < 2^24
    for (Bc, Cic, Co1, Co2, Mc, bias) in FWD_CASES + [(1, 512, 130, 0, 65, True), (3, 512, 40, 24, 3, False)]:
        for mode in ("int", "min", "ext"):
            if mode == "min" and Cic > 128 or mode == "ext" and Cic != 512:
                continue
            wi_, c_, dw_, b_, lo_, hi_ = fwd_operands(Bc, Cic, Co1, Co2, Mc, bias, mode, 100 + Cic + Co1 + Mc)
            s = torch.einsum("oc,bcm->bom", wi_.double().abs(), c_.double()) + (abs(lo_) * wi_.double().abs().sum(1))[None, :, None]
            assert exact_ok(s + (b_.abs().max() if b_ is not None else 0.0)), (Bc, Cic, Co1, Co2, Mc, mode)
    for (Bc, Cic, Co1, Co2, Mc, add) in DG_CASES:
        assert exact_ok(dg_abs(*dg_exact_operands(Bc, Cic, Co1 + Co2, Mc, add, 500 + Cic + Co1 + Co2 + Mc))), (Bc, Cic, Co1, Co2, Mc)
    for (Bc, Cic, Co1, Co2, Mc) in WG_CASES:
        gz_, c_, st_ = wg_exact_operands(Bc, Cic, Co1 + Co2, Mc, 700 + Cic + Co1 + Co2 + Mc)
        assert exact_ok(torch.einsum("bom,bcm->oc", gz_.double().abs(), c_.double() + 3) + st_.abs()), (Bc, Cic, Co1, Co2, Mc)
    # every value of every axis the issue names is in the grids
    ax = lambda cases, k: {c[k] for c in cases}
    assert ax(FWD_CASES, 1) == {16, 48, 128, 512} and {1, 33, 130, 512} <= ax(FWD_CASES, 2) and ax(FWD_CASES, 4) == {1, 3, 63, 64, 65, 130}
    assert {(c[2], c[3]) for c in FWD_CASES if c[3]} == {(40, 24), (16, 16), (128, 128), (96, 32)} and ax(FWD_CASES, 0) == {1, 3}
    assert {c[2] + c[3] for c in DG_CASES if not c[3]} == {16, 48, 512, 1024, 1040, 1536, 2064} and ax(DG_CASES, 1) == {1, 16, 130, 512}
    assert {(c[2], c[3]) for c in DG_CASES if c[3]} == {(48, 16), (32, 48), (512, 512)} and ax(DG_CASES, 4) == {1, 3, 63, 64, 65, 130}
    assert ax(WG_CASES, 4) == {1, 3, 63, 64, 65, 255, 256, 257, 1030} and {1, 64, 65, 200} <= ax(WG_CASES, 2)
    assert {(c[2], c[3]) for c in WG_CASES if c[3]} == {(48, 16), (128, 128), (144, 40)} and ax(WG_CASES, 1) == {16, 128, 130, 256, 300}
    assert ax(PW_CASES, 1) == {4, 20, 128, 432} and {(c[0], c[1], c[2]) for c in WQ_CASES} >= {(1, 16, 8), (33, 300, 4), (512, 512, 8)}
