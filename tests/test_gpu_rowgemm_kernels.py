"""The row-major GEMM kernels -- k_qrow_fwd (csrc/qrow.hip, int8 MFMA, three fused epilogues), the row entries of csrc/gemm.hip with
their two implementations k_gemm_x3 / k_gemm_f32<VEC = false>, the coded-B forms of csrc/gemm_x3.hip and k_gemm_x3_wq_multi -- at the C
ABI, against exact integers and float64.  The entry points are called through fqss_amd._lib with explicit pointers and leading dimensions,
in the manner of tests/test_gpu_qgemm_kernels.py (whose buffers and helpers this file imports).

Entry points covered: fqss_qrow_fwd, fqss_qrow_fwdq, fqss_qrow_fwdq2; fqss_rowlin_fwd, fqss_rowlin_fwd_w3 (+ fqss_split3_planes),
fqss_rowlin_bwd_x, fqss_rowlin_bwd_w, fqss_rowlin_bwd_w_batched, fqss_qrow_bwd_x, fqss_qrow_bwd_w, fqss_qrow_bwd_wb,
fqss_qrow_bwd_w_batched; fqss_qrow_bwd_w_group; and the deterministic-mode form of the row weight gradients' atomics.  Every entry has
guarded-buffer cases and one refusal per FQSS_REQUIRE that the flat ABI can reach (test_*_refusals).  Not reachable there: "batch >= 1"
of fqss_rowlin_bwd_w and the batch / problem-stride rules of fqss_qrow_bwd_w / _wb (those entries pass batch = 1 and zero strides
themselves); "unsupported operand layout" of launch_gemm and "coded data gradient: one problem per launch" of launch_gemm_x3q (the row
entries pass the layouts and batch = 1 themselves); "operands not eligible for the split-bf16 GEMM" of fqss_rowlin_fwd_w3 (the REQUIRE in
front of it -- Ci % 32, aligned x and w3, ld_x % 4 -- is everything x3_ok asks of that problem).

Layout under test.  fp32 operands sit in NaN-filled flat buffers between guard floats, row padding stays NaN; code operands sit in
0xA5-filled buffers between guard bytes; outputs are NaN- / 0xA5-filled, the accumulating ones (gw, gbias) start from non-zero random
values.  At least one operand of every case has padding beyond what its alignment rule asks for, and the operands of a case have different
ld's.  After each call: every operand bit-identical, the guards and everything outside the live elements untouched -- [R][Co] of z / y /
yc, [R][Ci] of gx, the Co x Ci of each gw, Co of gbias: no entry of this file writes a whole float4 past the last live column (the staged
epilogues of k_qrow_fwd and k_gemm_x3 finish a row with scalar stores; include/fqss.h says so since this file) -- and every live output
element finite.

Tile shapes.  launch_gemm_x3, launch_gemm_x3q, launch_gemm and fqss_qrow_bwd_w_group pick (MI, NI) from M, N and the grid; at this commit
the row entries reach (2, 1) [N <= 64], (1, 2) [N > 64 and M <= 64, or a grid below the 320- / 256-tile threshold] and (2, 2).  (1, 1)
is instantiated for the implicit convolutions only: with N <= 64 the rule keeps mi = 2 -- so "all tile shapes" below are these three.

Exact-integer cases (torch.equal, no tolerance).  k_qrow_fwd with dw = 1, rw = sum k, range [lo, lo + 255] (dx = 1): z = S + lo R + b is
an integer in every intermediate provided sum |k| |c - 128|, 128 sum |k|, |lo| sum |k| and |S|, |S + lo R|, |z| stay below 2^24
(qrow_exact_ok, asserted on the CPU per case); extreme codes (k in {-128, 127}, c in {0, 255}) satisfy it up to Ci = 1024, Ci = 2048 runs
with |k| <= 15.  The coded gradients with gz = n 2^-20 reach the second and third bf16 piece (asserted on the CPU) with dw in {1, 2}
(fqss_qrow_bwd_x) and dx = 1, lo = -3 (fqss_qrow_bwd_w / _wb).

Forward against float64 with real ranges: the bound is derived, not measured.  The kernel forms the exact int32 S' = sum k (c - 128), then
   S = fl(fl(S') + 128 R)    two roundings (the conversion above 2^24, the sum); the two terms cancel, so their errors are relative to
                             |S'| and |S'| + 128 |R|, not to |S|
   v = fl(dw fl(fl(dx S) + fl(lo R))) , z = fl(v + b)     five more
-- seven roundings, each at most 2^-24 of mag = |dw dx| (|S'| + 128 |R|) + |dw lo R| + |b| to first order; ROW_ULPS = 8 of them cover the
second-order terms:  |z - ref| <= 8 2^-24 mag per element, ref built from the integers S and R with dx the fp32 value of (hi - lo) / 255.
The staged and the scalar epilogue must agree bit for bit on the same operands.

Measured on the MI355X (two runs; the weight gradients go through fp32 atomics and differ from run to run): largest e_elem / e_norm over
a family's cases, beside torch fp32 on the CPU on the same cases, the bound
(BOUND below, at most 4 x the measurement) and its factor:
                                              kernel               fp32                 bound                factor
  k_qrow_fwd (all three entries)    z       <= 0.29 of the derived per-element bound (torch fp32 F.linear: up to 105 x that bound at Ci = 2048)
  x3 float      fqss_rowlin_fwd     z       1.91e-6 / 1.77e-7    1.61e-6 / 1.50e-7    6.7e-6 / 6.2e-7      3.5 / 3.5   (300, 256, 130)
                fqss_rowlin_bwd_x   gx      4.70e-6 / 2.44e-7    6.29e-6 / 2.05e-7    1.6e-5 / 8.5e-7      3.4 / 3.5   (33000, 130, 32)
                fqss_rowlin_bwd_w   gw      2.09e-6 / 2.96e-7    2.96e-6 / 7.17e-7    6.7e-6 / 1.0e-6      3.2 / 3.4   (4200, 256, 256); batched
                                                                                                           against its single launches 4.3e-7 / 3.5e-8; deterministic mode 9.2e-7 / 1.4e-7
  fallback      fqss_rowlin_fwd     z       1.90e-6 / 2.07e-7    1.61e-6 / 1.50e-7    6.6e-6 / 7.2e-7      3.5 / 3.5   (300, 256, 130)
  float         fqss_rowlin_bwd_x   gx      6.29e-6 / 2.80e-7    6.29e-6 / 2.05e-7    2.2e-5 / 9.8e-7      3.5 / 3.5   (33000, 130, 32)
                fqss_rowlin_bwd_w   gw      2.42e-6 / 3.51e-7    2.96e-6 / 7.17e-7    7.9e-6 / 9.5e-7      3.3 / 2.7   (63, 130, 130); batched
                                                                                                           against its single launches 1.9e-6 / 2.0e-7
  coded dgrad   fqss_qrow_bwd_x     gx      1.93e-6 / 1.66e-7    2.56e-6 / 2.11e-7    6.7e-6 / 5.8e-7      3.5 / 3.5   (257, 132, 256)
  coded wgrad   fqss_qrow_bwd_w/_wb gw      3.00e-6 / 2.10e-7    2.51e-6 / 2.16e-7    1.05e-5 / 7.3e-7     3.5 / 3.5   (257, 68, 200); deterministic
                / _batched                                                                                 mode 1.3e-6 / 2.0e-7
                fqss_qrow_bwd_wb    gbias   4.28e-7 / 1.11e-7    5.77e-7 / 1.16e-7    1.5e-6 / 3.9e-7      3.5 / 3.5   (257, 260, 132)
  group         fqss_qrow_bwd_w_    gw      3.58e-6 / 4.75e-7    (the coded wgrad's)  1.25e-5 / 1.66e-6    3.5 / 3.5   job (256, 132, 68); deterministic
                group               gbias   7.65e-7 / 1.80e-7                         2.7e-6 / 6.3e-7      3.5 / 3.5   mode 2.3e-6 / 3.7e-7
No family sits above its fp32 yardstick by more than a factor 1.4 (e_elem is a maximum over heavy-tailed gradients divided by an rms: it
sits an order above e_norm, for torch fp32 as for the kernels).
Bit-exact, no bound: every exact-integer case; the epilogue pair; fqss_qrow_fwdq's z against fqss_qrow_fwd and y against
oracle.act_quantize of the activated kernel z; fqss_qrow_fwdq2's y / yc against the oracle; fqss_rowlin_fwd_w3 against fqss_rowlin_fwd;
fqss_split3_planes; fqss_qrow_bwd_wb's gw against fqss_qrow_bwd_w where one k-slice adds (R <= 64); the jobs of one k-slice (R <= 256)
of fqss_qrow_bwd_w_group run to run; deterministic mode run to run.  The grouped kernel's order is NOT fixed where a job has more than
one k-slice: every slice adds its tile to gw (and its row sums to gbias) with fp32 atomics, in the order the workgroups retire -- that
run-to-run assertion is made for the single-slice jobs only and the others are held by the bound and by deterministic mode.

Mutation floors: e_elem of the wrong kernel, computed in float64 on the CPU on each case's own operands, asserted 10 x above the bound in
every non-void case (L.floor; for the forward the unit is the element's derived bound).  Smallest floor over the non-void cases:
  k_qrow_fwd   (in units of the element's bound, where 10 is asked) last k-tile dropped 2.2e6 (void at Ci <= 64: one tile); min_x R dropped
               3.1e5; dw of the neighbouring row 2.9e5 (void at Co = 1); padding column Ci read against a weight code of the rms 1.6e5.
               Exact cases, share of the elements that differ: last 16-byte k-chunk dropped 0.9998; 128 R dropped 1.0; rw of the
               neighbouring row 0.67 (Co = 3; void at Co = 1); the code of column Ci read 0.39
  float fwd    (x3 and fallback alike: the same operands) last k-tile (K <= 32: the last four k) dropped 0.16; bias / weight row of the
               neighbouring column 0.52 (void at Co = 1); padding column Ci read as values of the rms 4.5e-2
  float bwd_x  last k-tile dropped 1.7; weight column of the neighbouring output 7.8; padding column Co of gz read 6.3e-2
  float bwd_w  last k-tile dropped 0.14 (void at R <= 32); last live row dropped 2.2e-2 (R = 1030, Ci x Co = 4 x 1; void at R = 1); row R
               read as values of the rms 1.5e-2 (R = 4200, the most diluted case); batched: x of the other problem 9.7
  coded dgrad  last k-tile dropped 0.30; dw of the neighbouring row 8.7e-2; column index one off 2.2; padding column Co of gz read 4.4e-2
  coded wgrad  last k-tile dropped 0.44 (void at R <= 32); min_x row sum dropped 1.4; last live row dropped 0.44 (gbias: 0.24); row R read
               (gz of the rms, code 255) 0.13; gbias added once per column tile 2.4; batched: the other column block 6.0
  group        last k-tile dropped 0.40; min_x row sum dropped 1.9; last live row dropped 0.38 (gbias: 0.19); row R read 7.9e-2
  The third piece in the float64 cases, e_elem / e_norm over the cases: float 1.6e-5 .. 5.4e-4 / 5.0e-6 .. 1.9e-5, coded 5.3e-6 .. 1.3e-4
  / 1.9e-6 .. 1.5e-5.
  Void in the float64 cases: the third bf16 piece dropped (printed per case: it moves a product by at most 2^-16 of itself) -- over the
  bounds but not by the 10 x of a floor.  The bit-exact runs hold it instead: test_coded_dgrad_exact_through_the_bf16_pieces and
  test_coded_wgrad_exact_through_the_bf16_pieces assert on the CPU that their operands have non-zero second and third pieces and that a
  kernel without the piece differs; for the float x float form fqss_rowlin_fwd_w3 == fqss_rowlin_fwd and the exactness of
  fqss_split3_planes tie the on-the-fly split to the three stored planes.

Checked once on the MI355X against scratch copies of the library carrying ONE arithmetic mutation each (built outside the package, never
committed; no mutation changes an address): the zeroing of a k-chunk past Ci dropped in k_qrow_fwd -- 17 tests fail (every exact and
float64 case with Ci % 64 != 0); the mask k < kend of TileIO's k-contiguous store dropped -- 9 (the NaN padding of K = 30 / 70 reaches z
and gx, K % 32 != 0 re-adds clamped columns); the third bf16 piece dropped in x_split3 -- 50 (every float64 case of the split-bf16
families, both piece tests, fqss_rowlin_fwd_w3 against fqss_rowlin_fwd); the last two k of every 16-wide tile dropped in k_gemm_f32 -- 28
(every fallback run); gbias added by every column tile -- 7.  Void: the mask k < kend of TileIOQ's store dropped passes every test -- the A
tile is zero there, the codes it lets through are finite, and nothing of it reaches a result: that mask is redundant with TileIO's.

Defects found and fixed with this file:
  None.  Every case of this file passes on the library of the parent commit: the clamped loads of TileIO / TileIOQ / TileIOP and of
  k_qrow_fwd keep NaN row padding out of every result, the scalar fallback and the scalar epilogues compute what the vector paths
  compute, and no entry writes outside its live elements.  What the file adds to the header is documentation of that behaviour.

References: plain float64 torch on the CPU from the formulas in include/fqss.h; test_references_on_cpu ties them to float64 F.linear on
oracle.fqss_oracle.weight_quantize / act_quantize operands and to that graph's autograd.  e_elem = max |got - ref| / rms(ref), e_norm =
||got - ref|| / ||ref||; the yardstick is the same operation in torch fp32 on the CPU ("MEAS" lines)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import oracle.fqss_oracle as O
import tests.test_gpu_layout_spectral_kernels as L
from tests.test_gpu_layout_spectral_kernels import (DEV, EINVAL, F64, G, NAN, Blk, Vec, all_unchanged, errs, gpu, pad4, refused, rms,  # noqa: F401
                                                    stream)
from tests.test_gpu_qgemm_kernels import (GB, SENT, TWO24, ULP, Cod, act_cpu, codes, delta32, differs, exact_ok, f32, gen, heavy, ints,  # noqa: F401
                                          out_range, r4, r16, sc, split3, steps, wcodes)

K = None
_lib = None
ACT_NONE, ACT_PRELU, ACT_RELU, ACT_POST_RELU = 0, 1, 2, 4
ROW_ULPS = 8.0                           # derived (see above)
SLOPE = 0.2

# per family and tensor: (e_elem bound, e_norm bound), at most 4 x the largest figure measured on the MI355X over the family's cases
BOUND = {
    "x3": {"z": (6.7e-6, 6.2e-7), "gx": (1.6e-5, 8.5e-7), "gw": (6.7e-6, 1.0e-6)},
    "fb": {"z": (6.6e-6, 7.2e-7), "gx": (2.2e-5, 9.8e-7), "gw": (7.9e-6, 9.5e-7)},
    "qdx": {"gx": (6.7e-6, 5.8e-7)},
    "qdw": {"gw": (1.05e-5, 7.3e-7), "gb": (1.5e-6, 3.9e-7)},
    "group": {"gw": (1.25e-5, 1.66e-6), "gb": (2.7e-6, 6.3e-7)},
}


@pytest.fixture(scope="module")
def _gpu():
    global K, _lib
    L._gpu_fixture()
    K, _lib = L.K, L._lib
    yield


def call(name, *args):
    _lib.call(name, *args)
    torch.cuda.synchronize()


def measure(fam, name, got, ref, ref32, tag, fails):
    L.measure(fam, name, got, ref, ref32, tag, fails, bound=BOUND[fam][name])


def floor(fam, name, mut, ref, what, tag):
    L.floor(fam, name, mut, ref, what, tag, bound=BOUND[fam][name])


def third_piece(fam, name, mut, ref, tag):
    fl = errs(mut, ref)
    print(f"FLOOR {fam} {name} third bf16 piece dropped {fl[0]:.2e} / {fl[1]:.2e} (bound {BOUND[fam][name]}; void here, see the docstring) | {tag}")


def ptr(v):
    return v.ptr if v is not None else None


class Flat:
    """n NaN floats between guards, operands placed at element offsets (batched problems, arenas of views)"""

    def __init__(self, n):
        self.v = Vec(n)
        self.live = torch.zeros_like(self.v.buf, dtype=torch.bool)

    def view(self, off, R, M, ld):
        return self.v.buf.as_strided((R, M), (ld, 1), G + off)

    def put(self, off, t, ld):
        self.view(off, t.shape[0], t.shape[1], ld).copy_(t)
        return self

    def mark(self, off, R, M, ld):
        """[R][M] at `off` is an output's live region"""
        self.live.as_strided((R, M), (ld, 1), G + off).fill_(True)

    def snap(self):
        self.v.before = self.v.buf.clone()

    def at(self, off):
        return self.v.buf.data_ptr() + 4 * (G + off)

    def unchanged(self):
        return self.v.unchanged()

    def only_live_changed(self):
        keep = ~self.live
        return bool(torch.equal(L._bits(self.v.buf)[keep], L._bits(self.v.before)[keep]))

    def cpu(self, off, R, M, ld):
        return self.view(off, R, M, ld).cpu().contiguous()


# ------------------------------------------------------------------------------------------------------------- references (float64)
def lin_ref(x, w, b=None):
    z = x.double() @ w.double().t()
    return z + b.double() if b is not None else z


def dx_ref(gz, w):
    return gz.double() @ w.double()


def dw_ref(gz, x):
    return gz.double().t() @ x.double()


def qfwd_parts(wi, c, dw, b, lo, hi):
    """S' = sum k (c - 128), R = sum k, the three terms of z = dw (dx S + min_x R) + b and mag, the magnitude the derived bound is stated
    in -- all in float64, dx the fp32 step"""
    Sp = (c.double() - 128.0) @ wi.double().t()
    Rk = wi.double().sum(1)
    dx, mn = delta32(lo, hi).double(), f32(lo).double()
    dwd = dw.double()
    t1 = dwd * dx * (Sp + 128.0 * Rk)
    t2 = (dwd * mn * Rk).expand_as(Sp)
    t3 = (b.double() if b is not None else torch.zeros(wi.shape[0], dtype=F64)).expand_as(Sp)
    mag = (dwd * dx).abs() * (Sp.abs() + 128.0 * Rk.abs()) + t2.abs() + t3.abs()
    return Sp, Rk, t1, t2, t3, mag


def qfwd_ref(wi, c, dw, b, lo, hi):
    _, _, t1, t2, t3, _ = qfwd_parts(wi, c, dw, b, lo, hi)
    return t1 + t2 + t3


def qdx_ref(gz, wi, dw):
    """gx = gz W_q, W_q = dw[o] wi[o][i]"""
    return gz.double() @ (wi.double() * dw.double()[:, None])


def qdw_ref(gz, c, lo, hi, dropmin=False):
    """gw[o][i] = sum_r gz[r][o] (dx c[r][i] + min_x)"""
    dx, mn = delta32(lo, hi).double(), f32(lo).double()
    gw = dx * (gz.double().t() @ c.double())
    return gw if dropmin else gw + mn * gz.double().sum(0)[:, None]


def floor_fwd(mut, ref, bnd, what, tag):
    """forward: the wrong kernel `what` misses the derived per-element bound by 10 x somewhere"""
    fl = float(((mut - ref).abs() / bnd.clamp_min(1e-300)).max())
    print(f"FLOOR qrow z {what} {fl:.2e} x the element's bound | {tag}")
    assert fl >= 10, (tag, what, fl)


# ============================================================================================================ 1. - 4. k_qrow_fwd
# (R, Ci, Co, padding of the code rows beyond Ci, layout of z, bias).  z: "st" 16-B rows (the LDS-staged epilogue), "odd" an odd ld_z,
# "off" z one float off a 16-B boundary (both: the scalar epilogue)
QROW_CASES = [(1, 16, 1, 0, "st", True), (31, 32, 3, 16, "odd", False), (33, 48, 33, 48, "st", True), (127, 64, 64, 0, "off", True),
              (128, 80, 65, 16, "st", False),      # Co % 4 != 0 behind two whole sub-tiles
              (129, 256, 96, 48, "st", True),      # Co in (64, 96]: the fourth 32-column sub-tile is skipped (ob >= Co)
              (257, 1024, 130, 0, "st", True), (33, 2048, 192, 16, "st", False),      # the documented maximum of Ci
              (129, 48, 130, 16, "odd", True), (257, 80, 192, 48, "off", False), (31, 1024, 65, 48, "odd", True), (128, 16, 96, 16, "st", False),
              (1, 256, 3, 0, "st", True), (127, 32, 33, 0, "odd", False)]
OTHER = {"st": "odd", "odd": "st", "off": "st"}
# (R, Ci, Co, act, layout of z, layout of y)
FWDQ_CASES = [(33, 48, 33, ACT_NONE, "st", "st"), (129, 80, 130, ACT_RELU, "st", "st"), (128, 64, 65, ACT_PRELU, "st", "st"),
              (257, 32, 96, ACT_POST_RELU, "st", "st"), (33, 48, 33, ACT_POST_RELU, "odd", "st"), (129, 80, 130, ACT_PRELU, "st", "off"),
              (128, 64, 65, ACT_RELU, "off", "odd"), (257, 32, 96, ACT_NONE, "st", "odd")]
FWDQ2_CASES = [(129, 80, 192), (33, 48, 64), (257, 32, 132)]


def qrow_operands(R, Ci, Co, bias, mode, seed):
    """mode "int": dw = 1, range [0, 255], integer bias (|k| <= 15 at Ci = 2048); "min": the same with range [-3, 252]; "ext": k in
    {-128, 127}, c in {0, 255}; "real": real steps and ranges"""
    g = gen(seed)
    wi, c = wcodes(g, Co, Ci, lim=16 if (Ci > 1024 and mode != "real") else 128), codes(g, R, Ci)
    if mode == "ext":
        wi = torch.where(torch.rand(Co, Ci, generator=g) < 0.5, -128, 127).to(torch.int8)
        c = torch.where(torch.rand(R, Ci, generator=g) < 0.5, 0, 255).to(torch.uint8)
    if mode == "real":
        dw, lo, hi = steps(g, Co), -0.731, 1.913
        b = torch.randn(Co, generator=g) * 0.5 if bias else None
    else:
        dw, (lo, hi) = torch.ones(Co), ((-3.0, 252.0) if mode == "min" else (0.0, 255.0))
        b = ints(g, 1000, Co) if bias else None
    return wi, c, dw, b, lo, hi


def qrow_exact_ok(wi, c, b, lo):
    """every intermediate of z = S + lo R + b is an integer below 2^24"""
    k, cd = wi.double(), c.double()
    a1 = (cd - 128.0).abs() @ k.abs().t()
    a2, a3 = 128.0 * k.abs().sum(1), abs(lo) * k.abs().sum(1)
    S, Rk = cd @ k.t(), k.sum(1)
    tot = S + lo * Rk
    return exact_ok(a1, a2, a3, S.abs(), tot.abs(), (tot + (b.double() if b is not None else 0.0)).abs())


def zblk(R, Co, lay, extra=8):
    if lay == "st":
        return Blk(R, Co, r4(Co) + extra)
    if lay == "odd":
        return Blk(R, Co, r4(Co) + extra + 1)
    return Blk(R, Co, r4(Co) + extra, off=1)


class QRowOps:
    """the device operands of one k_qrow_fwd case"""

    def __init__(self, R, Ci, Co, xpad, wi, c, dw, b, lo, hi):
        self.dims = (R, Ci, Co)
        self.xc, self.wk = Cod(R, Ci, Ci + xpad, fill=c), Cod(Co, Ci, fill=wi)
        self.dw, self.rw = Vec(Co, fill=dw), Vec(Co, fill=wi.double().sum(1))
        self.b = Vec(Co, fill=b) if b is not None else None
        self.lo, self.hi = sc(lo), sc(hi)

    def unchanged(self):
        ops = dict(xc=self.xc, wk=self.wk, dw=self.dw, rw=self.rw, lo=self.lo, hi=self.hi)
        if self.b is not None:
            ops["b"] = self.b
        all_unchanged(**ops)

    def head(self):
        return [self.xc.ptr, self.wk.ptr, self.dw.ptr, self.rw.ptr, ptr(self.b), self.lo.ptr, self.hi.ptr]

    def fwd(self, lay):
        R, Ci, Co = self.dims
        z = zblk(R, Co, lay)
        call("fqss_qrow_fwd", *self.head(), z.ptr, R, Ci, Co, self.xc.ld, z.ld, stream())
        self.unchanged()
        assert z.written(), "fqss_qrow_fwd wrote outside [R][Co] (or left a live element)"
        return z.cpu(R, Co)

    def fwdq(self, lay_z, lay_y, act, slope, rng):
        R, Ci, Co = self.dims
        z, y = zblk(R, Co, lay_z), zblk(R, Co, lay_y, extra=16)
        assert y.ld != z.ld
        sl, r = (sc(slope) if slope is not None else None), [sc(v) for v in rng]
        call("fqss_qrow_fwdq", *self.head(), z.ptr, y.ptr, R, Ci, Co, self.xc.ld, z.ld, y.ld, act, ptr(sl), r[0].ptr, r[1].ptr, stream())
        self.unchanged()
        all_unchanged(**{f"r{i}": v for i, v in enumerate(r + [sl]) if v is not None})
        assert z.written() and y.written(), "fqss_qrow_fwdq wrote outside [R][Co]"
        return z.cpu(R, Co), y.cpu(R, Co)

    def fwdq2(self, r1, r2):
        R, Ci, Co = self.dims
        z, y = Blk(R, Co, Co + 8), Blk(R, Co, Co + 4)
        yc = Cod(R, Co, Co + 12, off=4)                   # (4-B aligned only)
        r = [sc(v) for v in (*r1, *r2)]
        call("fqss_qrow_fwdq2", *self.head(), z.ptr, y.ptr, yc.ptr, R, Ci, Co, self.xc.ld, z.ld, y.ld, yc.ld, *[v.ptr for v in r], stream())
        self.unchanged()
        all_unchanged(**{f"r{i}": v for i, v in enumerate(r)})
        assert z.written() and y.written() and yc.written(), "fqss_qrow_fwdq2 wrote outside [R][Co]"
        return z.cpu(R, Co), y.cpu(R, Co), yc.cpu(R, Co)


def qrow_exact(case, mode, seed):
    R, Ci, Co, xpad, lay, bias = case
    wi, c, dw, b, lo, hi = qrow_operands(R, Ci, Co, bias, mode, seed)
    assert float(delta32(lo, hi)) == 1.0 and qrow_exact_ok(wi, c, b, lo), (case, mode)
    ref = qfwd_ref(wi, c, dw, b, lo, hi).float()
    ops = QRowOps(R, Ci, Co, xpad, wi, c, dw, b, lo, hi)
    for ly in (lay, OTHER[lay]):
        assert torch.equal(ops.fwd(ly), ref), (case, mode, ly)
    return wi, c, b, lo, xpad


def qrow_mutations(wi, c, b, lo, xpad, tag):
    """a differing-element count for each wrong kernel, on the exact case's own operands"""
    k, cd = wi.double(), c.double()
    R, Ci = c.shape
    bb = b.double() if b is not None else 0.0
    Rk = k.sum(1)
    ref = cd @ k.t() + lo * Rk + bb
    Sp = (cd - 128.0) @ k.t()
    differs((cd[:, :Ci - 16] - 128.0) @ k[:, :Ci - 16].t() + 128.0 * Rk + lo * Rk + bb, ref, "last 16-byte k-chunk dropped", tag)
    differs(Sp + lo * Rk + bb, ref, "128 R dropped", tag)
    if wi.shape[0] > 1:
        differs(Sp + (128.0 + lo) * Rk.roll(1) + bb, ref, "rw of the neighbouring row", tag)
    # the chunk one column late: the code of column Ci (row padding, or the next row's first code where ld_x = Ci) in place of column Ci - 1
    flat = torch.full((R * (Ci + xpad) + 1,), float(SENT), dtype=F64)
    flat[:-1].view(R, Ci + xpad)[:, :Ci] = cd
    nxt = flat[torch.arange(R) * (Ci + xpad) + Ci]
    differs(ref + (nxt - cd[:, Ci - 1])[:, None] * k[:, Ci - 1][None, :], ref, "the code of column Ci read", tag)


@gpu
@pytest.mark.parametrize("case", QROW_CASES, ids=str)
def test_qrow_forward_exact_integers(case):
    """fqss_qrow_fwd with dw = 1, dx = 1, an integer min_x (0 / -3 by turns) and integer bias: z is the integer sum bit for bit, in both
    epilogues"""
    R, Ci, Co = case[:3]
    k = QROW_CASES.index(case)
    wi, c, b, lo, xpad = qrow_exact(case, "min" if k % 2 else "int", 100 + k)
    qrow_mutations(wi, c, b, lo, xpad, f"qrow exact {case}")


@gpu
def test_qrow_forward_exact_integers_extreme_codes():
    """k in {-128, 127}, c in {0, 255} up to Ci = 1024: |S'| and 128 |R| just below 2^24"""
    for k, case in enumerate([(129, 1024, 130, 16, "st", True), (33, 1024, 65, 0, "odd", False), (31, 80, 3, 48, "st", True)]):
        wi, c, b, lo, xpad = qrow_exact(case, "ext", 150 + k)
        qrow_mutations(wi, c, b, lo, xpad, f"qrow extreme {case}")


@gpu
@pytest.mark.parametrize("case", QROW_CASES, ids=str)
def test_qrow_forward_against_fp64(case):
    """real steps and ranges: every element within 8 x 2^-24 mag of the float64 value; the two epilogues agree bit for bit"""
    R, Ci, Co, xpad, lay, bias = case
    wi, c, dw, b, lo, hi = qrow_operands(R, Ci, Co, bias, "real", 200 + QROW_CASES.index(case))
    ops = QRowOps(R, Ci, Co, xpad, wi, c, dw, b, lo, hi)
    z = ops.fwd(lay)
    assert torch.equal(z, ops.fwd(OTHER[lay])), "the staged and the scalar epilogue differ"
    Sp, Rk, t1, t2, t3, mag = qfwd_parts(wi, c, dw, b, lo, hi)
    ref, bnd = t1 + t2 + t3, ROW_ULPS * ULP * mag
    z32 = F.linear(delta32(lo, hi) * c.float() + f32(lo), dw[:, None] * wi.float(), b)
    tag = f"qrow {case}"
    worst, worst32 = float(((z.double() - ref).abs() / bnd).max()), float(((z32.double() - ref).abs() / bnd).max())
    print(f"MEAS qrow z {worst:.2f} of the element's bound, torch fp32 {worst32:.2f} | {tag}")
    assert worst <= 1.0, (tag, worst)
    if Ci > 64:
        kl = (Ci - 1) // 64 * 64
        floor_fwd(qfwd_ref(wi[:, :kl], c[:, :kl], dw, b, lo, hi) + (dw.double() * f32(lo).double() * wi[:, kl:].double().sum(1)), ref, bnd,
                  "last k-tile dropped", tag)
    floor_fwd(t1 + t3, ref, bnd, "min_x R dropped", tag)
    if Co > 1:
        floor_fwd(qfwd_ref(wi, c, dw.roll(1), b, lo, hi), ref, bnd, "dw of the neighbouring row", tag)
    pad_code = torch.full((R, 1), SENT, dtype=torch.uint8)
    krms = torch.full((Co, 1), max(1, round(rms(wi))), dtype=torch.int8)
    floor_fwd(qfwd_ref(torch.cat([wi, krms], 1), torch.cat([c, pad_code], 1), dw, b, lo, hi) - (dw.double() * f32(lo).double() * krms[:, 0].double()),
              ref, bnd, "padding column Ci read (against a code of the rms)", tag)


def fwdq_ranges(zref, act):
    """the output range of a fused-quantizer case from the float64 reference z: the quartiles of the activated z (of z itself where the
    ReLU sits behind the quantizer; of the positive values behind a ReLU, half of whose outputs are zero) -- a visible share of the
    elements saturates at either end"""
    t = zref.float() if act == ACT_POST_RELU else act_cpu(zref.float(), act, SLOPE)
    return out_range(t[t > 0] if act == ACT_RELU else t), t


def shares(t, r):
    lo, hi = f32(r[0]), f32(r[1])
    return float((t < lo).float().mean()), float(((t >= lo) & (t <= hi)).float().mean()), float((t > hi).float().mean())


def fwdq2_ranges(zref):
    r1 = out_range(zref.float())
    t = torch.relu(O.act_quantize(zref.float(), f32(r1[0]), f32(r1[1])))
    return r1, (0.15 * r1[1], 0.8 * r1[1]), t


@gpu
@pytest.mark.parametrize("case", FWDQ_CASES, ids=str)
def test_qrow_fused_quantizer(case):
    """fqss_qrow_fwdq: z bit-equal to fqss_qrow_fwd, y bit-equal to oracle.act_quantize of the activated kernel z (POST_RELU: relu of
    act_quantize(z)), through both epilogues, ld_y != ld_z"""
    R, Ci, Co, act, lz, ly = case
    wi, c, dw, b, lo, hi = qrow_operands(R, Ci, Co, True, "real", 300 + FWDQ_CASES.index(case))
    ops = QRowOps(R, Ci, Co, 16, wi, c, dw, b, lo, hi)
    rng, _ = fwdq_ranges(qfwd_ref(wi, c, dw, b, lo, hi), act)
    plain = ops.fwd(lz)
    z, y = ops.fwdq(lz, ly, act, SLOPE if act == ACT_PRELU else None, rng)
    assert torch.equal(z, plain)
    qlo, qhi = f32(rng[0]), f32(rng[1])
    if act == ACT_POST_RELU:
        want = torch.relu(O.act_quantize(z, qlo, qhi))
    else:
        want = O.act_quantize(act_cpu(z, act, f32(SLOPE)), qlo, qhi)
    assert torch.equal(y, want), (case, int((y != want).sum()))
    s = shares(z if act == ACT_POST_RELU else act_cpu(z, act, SLOPE), rng)
    assert min(s) > 0.1, (case, s)


@gpu
@pytest.mark.parametrize("case", FWDQ2_CASES, ids=str)
def test_qrow_fused_quantizer_pair(case):
    """fqss_qrow_fwdq2: z of fqss_qrow_fwd, y = fq2(relu(fq1(z))) and yc = oracle.act_indices of the same, bit for bit; ld_yc != ld_y, yc
    4-B aligned only"""
    R, Ci, Co = case
    wi, c, dw, b, lo, hi = qrow_operands(R, Ci, Co, True, "real", 350 + Ci)
    ops = QRowOps(R, Ci, Co, 48, wi, c, dw, b, lo, hi)
    r1, r2, _ = fwdq2_ranges(qfwd_ref(wi, c, dw, b, lo, hi))
    z, y, yc = ops.fwdq2(r1, r2)
    assert torch.equal(z, ops.fwd("st"))
    t = torch.relu(O.act_quantize(z, f32(r1[0]), f32(r1[1])))
    assert torch.equal(y, O.act_quantize(t, f32(r2[0]), f32(r2[1])))
    assert torch.equal(yc, O.act_indices(t, f32(r2[0]), f32(r2[1])))
    assert min(shares(z, r1)) > 0.1 and min(shares(t, r2)) > 0.1 and int(yc.min()) == 0 and int(yc.max()) == 255


@gpu
def test_qrow_forward_refusals():
    """each FQSS_REQUIRE of the three forwards; no output is touched; R = 0 is a no-op"""
    R, Ci, Co = 5, 32, 8
    g = gen(5)
    xc, xo = [Cod(R, 2064, 2064, off=o, fill=torch.zeros(R, 2064, dtype=torch.uint8)) for o in (0, 8)]
    wk, wo = [Cod(Co, 2064, off=o, fill=torch.zeros(Co, 2064, dtype=torch.int8)) for o in (0, 4)]
    dw, rw, b, lo, hi = Vec(Co, fill=1.0), Vec(Co, fill=0.0), Vec(Co, fill=0.0), sc(0.0), sc(255.0)
    z, zo, y, yo = Blk(R, Co, 12), Blk(R, Co, 12, off=1), Blk(R, Co, 16), Blk(R, Co, 16, off=2)
    yc, yco = Cod(R, Co, 12), Cod(R, Co, 12, off=2)
    r, sl = [sc(-1.0), sc(1.0), sc(0.2), sc(0.8)], sc(0.2)
    S = stream()

    def fwd(xc_=xc.ptr, wk_=wk.ptr, dw_=dw.ptr, rw_=rw.ptr, lo_=lo.ptr, hi_=hi.ptr, z_=z.ptr, R=R, Ci=Ci, Co=Co, ldx=2064, ldz=12):
        refused("fqss_qrow_fwd", xc_, wk_, dw_, rw_, b.ptr, lo_, hi_, z_, R, Ci, Co, ldx, ldz, S)
        refused("fqss_qrow_fwdq", xc_, wk_, dw_, rw_, b.ptr, lo_, hi_, z_, y.ptr, R, Ci, Co, ldx, ldz, 16, ACT_NONE, None, r[0].ptr, r[1].ptr, S)
        refused("fqss_qrow_fwdq2", xc_, wk_, dw_, rw_, b.ptr, lo_, hi_, z_, y.ptr, yc.ptr, R, Ci, Co, ldx, ldz, 16, 12, *[v.ptr for v in r], S)

    def fwdq(y_=y.ptr, ldy=16, act=ACT_NONE, slope=None, q0=r[0].ptr, q1=r[1].ptr):
        refused("fqss_qrow_fwdq", xc.ptr, wk.ptr, dw.ptr, rw.ptr, b.ptr, lo.ptr, hi.ptr, z.ptr, y_, R, Ci, Co, 2064, 12, ldy, act, slope, q0, q1, S)

    def fwdq2(z_=z.ptr, y_=y.ptr, yc_=yc.ptr, Co=Co, ldz=12, ldy=16, ldyc=12, q=None):
        q = [v.ptr for v in r] if q is None else q
        refused("fqss_qrow_fwdq2", xc.ptr, wk.ptr, dw.ptr, rw.ptr, b.ptr, lo.ptr, hi.ptr, z_, y_, yc_, R, Ci, Co, 2064, ldz, ldy, ldyc, *q, S)

    for k in ("xc_", "wk_", "dw_", "rw_", "lo_", "hi_", "z_"):                            # null tensor
        fwd(**{k: None})
    fwd(R=-1)
    fwd(Ci=0)
    fwd(Ci=24)                                                                            # Ci % 16
    fwd(Ci=2064)                                                                          # Ci > 2048
    fwd(Co=0)
    fwd(Ci=2048, ldx=2032)                                                                # ld_x < Ci
    fwd(ldx=2056)                                                                         # ld_x % 16
    fwd(ldz=4)                                                                            # ld_z < Co
    fwd(xc_=xo.ptr)                                                                       # unaligned code images
    fwd(wk_=wo.ptr)
    fwdq(y_=None)
    fwdq(q0=None)
    fwdq(q1=None)
    fwdq(ldy=4)
    fwdq(act=ACT_PRELU)                                                                   # PReLU without a slope
    fwdq(act=3)                                                                           # GELU / RELU_Q / unknown: not this entry's
    fwdq(act=5)
    fwdq(act=9)
    fwdq2(yc_=None)
    for k in range(4):
        q = [v.ptr for v in r]
        q[k] = None
        fwdq2(q=q)
    fwdq2(Co=6)                                                                           # Co % 4
    fwdq2(ldy=4)
    fwdq2(ldyc=4)
    fwdq2(z_=zo.ptr)                                                                      # output rows 16-B, code rows 4-B aligned
    fwdq2(y_=yo.ptr)
    fwdq2(ldz=13)
    fwdq2(ldy=17)
    fwdq2(yc_=yco.ptr)
    fwdq2(ldyc=14)
    for o in (z, zo, y, yo, yc, yco):
        assert o.untouched()
    h = [xc.ptr, wk.ptr, dw.ptr, rw.ptr, b.ptr, lo.ptr, hi.ptr]
    call("fqss_qrow_fwd", *h, z.ptr, 0, Ci, Co, 2064, 12, S)
    call("fqss_qrow_fwdq", *h, z.ptr, y.ptr, 0, Ci, Co, 2064, 12, 16, ACT_NONE, None, r[0].ptr, r[1].ptr, S)
    call("fqss_qrow_fwdq2", *h, z.ptr, y.ptr, yc.ptr, 0, Ci, Co, 2064, 12, 16, 12, *[v.ptr for v in r], S)
    assert z.untouched() and y.untouched() and yc.untouched()


# ============================================================================================================== 5. float row GEMMs
# (R, Ci, Co): the instantiation of k_gemm_x3<true, true, false, MI, NI> the x3-eligible run is meant to reach (the fallback runs of
# the same shape reach k_gemm_f32<true, true, false, false, MI, NI> by launch_gemm's own rule, noted where it differs)
LIN_FWD = [(1, 4, 1),            # (2, 1): N <= 64; K < 32, one ragged k-tile
           (33, 20, 3),          # (2, 1); K = 20 < 32
           (129, 48, 33),        # (2, 1), two row tiles; K = 32 + 16
           (64, 32, 65),         # (1, 2): M <= 64, N > 64
           (127, 80, 130),       # (2, 2): 64 < M <= 128; K = 2 x 32 + 16
           (300, 256, 130),      # (1, 2): M > 128, 3 x 2 = 6 tiles < 320 (fallback: (1, 2), < 512)
           (41000, 32, 130),     # (2, 2): 321 x 2 = 642 tiles >= 320 (fallback: (2, 2), >= 512)
           (65, 30, 65),         # (2, 2); K = 30: not a multiple of 4 (the two NaN floats of the padded row), < 32
           (129, 70, 33)]        # (2, 1); K = 2 x 32 + 6: several k-tiles and a ragged one that ends inside a float4
# (R, Ci, Co) with N = Ci, K = Co: k_gemm_x3<true, false, false, MI, NI> (threshold 256 tiles)
LIN_BWDX = [(129, 33, 48),       # (2, 1): N = 33 <= 64 (w rows padded to 36)
            (64, 65, 32),        # (1, 2)
            (127, 130, 80),      # (2, 2)
            (300, 130, 256),     # (1, 2): 6 tiles < 256
            (33000, 130, 32),    # (2, 2): 258 x 2 = 516 tiles >= 256 (fallback: (2, 2), >= 512)
            (65, 68, 30),        # (2, 2); K = 30
            (129, 33, 70)]       # (2, 1); K = 70
# (R, Ci, Co) with M = Co, N = Ci, K = R: k_gemm_x3<false, false, true, MI, NI>; k-slices = ceil(R / kchunk), kchunk = 64 roundup(R / want)
LIN_BWDW = [(1, 4, 1), (1030, 4, 1),              # (2, 1); 1 and 17 slices (ragged last: 1030 = 16 x 64 + 6)
            (63, 20, 33), (257, 20, 33),          # (2, 1); 1 and 5 slices
            (65, 64, 130), (1030, 64, 130),       # (2, 1) with two row tiles; want = 128: 2 and 17 slices
            (130, 130, 33), (1, 130, 33),         # (1, 2): N > 64, M <= 64; want = 128: 3 and 1 slices
            (257, 130, 130), (63, 130, 130),      # (2, 2): four tiles, want = 64: 5 and 1 slices
            (1030, 65, 200), (130, 65, 200),      # (2, 2): M, N > 64 keeps 128 rows; want = 128: 17 and 3 slices
            (4200, 256, 256)]                     # (2, 2): want = 64 -> kchunk = 128, 33 slices


def lay(n, kind, extra=4):
    """(ld, offset in floats) of an operand with rows of n floats: "x3" 16-B rows with padding beyond the round-up; "odd" a row stride
    with ld % 4 = 1; "off" one float off a 16-B boundary"""
    return {"x3": (r4(n) + extra, 0), "odd": (r4(n) + extra + 1, 0), "off": (r4(n) + extra, 1)}[kind]


def lin_fwd_run(x, w, b, kind, zodd, entry="fqss_rowlin_fwd", w3=None):
    """kind "x3": every operand eligible for k_gemm_x3; "odd" / "off": x (odd) or w (off) is not -- k_gemm_f32<VEC = false>.  zodd: an odd
    ld_z (the scalar store epilogue of k_gemm_x3) instead of 16-B rows (the staged one)"""
    R, Ci = x.shape
    Co = w.shape[0]
    xb = Blk(R, Ci, *lay(Ci, "odd" if kind == "odd" else "x3"), fill=x)
    wb = Blk(Co, Ci, *lay(Ci, "off" if kind == "off" else "x3", 8), fill=w)
    bv = Vec(Co, fill=b) if b is not None else None
    z = Blk(R, Co, r4(Co) + (13 if zodd else 12))
    ops = dict(x=xb, w=wb)
    if bv is not None:
        ops["b"] = bv
    if w3 is None:
        call(entry, xb.ptr, wb.ptr, ptr(bv), z.ptr, R, Ci, Co, xb.ld, wb.ld, z.ld, stream())
    else:
        call("fqss_rowlin_fwd_w3", xb.ptr, w3.ptr, ptr(bv), z.ptr, R, Ci, Co, xb.ld, z.ld, stream())
    all_unchanged(**ops)
    assert z.written(), "fqss_rowlin_fwd wrote outside [R][Co] (or left a live element)"
    return z.cpu(R, Co)


def lin_bwdx_run(gz, w, kind, zodd):
    R, Co = gz.shape
    Ci = w.shape[1]
    gb = Blk(R, Co, *lay(Co, "odd" if kind == "odd" else "x3", 8), fill=gz)
    wb = Blk(Co, Ci, *lay(Ci, "off" if kind == "off" else "x3"), fill=w)
    gx = Blk(R, Ci, r4(Ci) + (13 if zodd else 12))
    call("fqss_rowlin_bwd_x", gb.ptr, wb.ptr, gx.ptr, R, Ci, Co, gb.ld, wb.ld, gx.ld, stream())
    all_unchanged(gz=gb, w=wb)
    assert gx.written(), "fqss_rowlin_bwd_x wrote outside [R][Ci]"
    return gx.cpu(R, Ci)


def lin_bwdw_run(gz, x, start, kind):
    R, Co = gz.shape
    Ci = x.shape[1]
    gb = Blk(R, Co, *lay(Co, "odd" if kind == "odd" else "x3"), fill=gz)
    xb = Blk(R, Ci, *lay(Ci, "off" if kind == "off" else "x3", 8), fill=x)
    gw = Blk(Co, Ci, Ci + 3, fill=start)
    call("fqss_rowlin_bwd_w", gb.ptr, xb.ptr, gw.ptr, R, Ci, Co, gb.ld, xb.ld, gw.ld, stream())
    all_unchanged(gz=gb, x=xb)
    assert gw.written(), "fqss_rowlin_bwd_w wrote outside the Co x Ci of gw"
    return gw.cpu(Co, Ci)


def lin_operands(R, Ci, Co, seed):
    g = gen(seed)
    x, w = torch.randn(R, Ci, generator=g), torch.randn(Co, Ci, generator=g) * Ci ** -0.5
    return x, w, torch.randn(Co, generator=g), heavy(g, R, Co)


def kinds(k):
    """the fallback reached through an odd ld in every case, through a base one float off in every other one"""
    return ("x3", "odd", "off") if k % 2 == 0 else ("x3", "odd")


@gpu
@pytest.mark.parametrize("case", LIN_FWD, ids=str)
def test_rowlin_forward_against_fp64(case):
    """fqss_rowlin_fwd through k_gemm_x3 (staged and scalar store epilogue by turns) and through the k_gemm_f32 fallback"""
    R, Ci, Co = case
    k = LIN_FWD.index(case)
    x, w, b, _ = lin_operands(R, Ci, Co, 400 + k)
    b = b if k % 3 else None
    ref, r32 = lin_ref(x, w, b), F.linear(x, w, b)
    fails, tag = [], f"rowlin fwd {case}"
    for kind in kinds(k):
        fam = "x3" if kind == "x3" else "fb"
        measure(fam, "z", lin_fwd_run(x, w, b, kind, zodd=k % 2 == 1), ref, r32, f"{tag} {kind}", fails)
        kl = (Ci - 1) // 32 * 32 if Ci > 32 else Ci - min(4, Ci - 1)
        if Ci > 1:
            floor(fam, "z", lin_ref(x[:, :kl], w[:, :kl], b), ref, "last k-tile (K <= 32: the last four k) dropped", tag)
        if Co > 1:
            floor(fam, "z", lin_ref(x, w, b.roll(1)) if b is not None else lin_ref(x, w.roll(1, 0)), ref, "bias / weight row of the neighbouring column", tag)
        floor(fam, "z", lin_ref(torch.cat([x, torch.full((R, 1), rms(x))], 1), torch.cat([w, torch.full((Co, 1), rms(w))], 1), b), ref,
              "padding column Ci read (values of the rms)", tag)
    h1, h2, _ = split3(x)
    third_piece("x3", "z", lin_ref(h1 + h2, w, b), ref, tag)
    assert not fails, fails


@gpu
@pytest.mark.parametrize("case", LIN_BWDX, ids=str)
def test_rowlin_data_gradient_against_fp64(case):
    """fqss_rowlin_bwd_x (heavy-tailed gz) through k_gemm_x3 and the fallback"""
    R, Ci, Co = case
    k = LIN_BWDX.index(case)
    _, w, _, gz = lin_operands(R, Ci, Co, 500 + k)
    ref, r32 = dx_ref(gz, w), gz @ w
    fails, tag = [], f"rowlin bwd_x {case}"
    for kind in kinds(k):
        fam = "x3" if kind == "x3" else "fb"
        measure(fam, "gx", lin_bwdx_run(gz, w, kind, zodd=k % 2 == 0), ref, r32, f"{tag} {kind}", fails)
        kl = (Co - 1) // 32 * 32 if Co > 32 else Co - 4
        floor(fam, "gx", dx_ref(gz[:, :kl], w[:kl]), ref, "last k-tile (K <= 32: the last four k) dropped", tag)
        floor(fam, "gx", dx_ref(gz, w.roll(1, 1)), ref, "weight column of the neighbouring output", tag)
        floor(fam, "gx", dx_ref(torch.cat([gz, torch.full((R, 1), rms(gz))], 1), torch.cat([w, torch.full((1, Ci), rms(w))], 0)), ref,
              "padding column Co of gz read (values of the rms)", tag)
    h1, h2, _ = split3(gz)
    third_piece("x3", "gx", dx_ref(h1 + h2, w), ref, tag)
    assert not fails, fails


@gpu
@pytest.mark.parametrize("case", LIN_BWDW, ids=str)
def test_rowlin_weight_gradient_against_fp64(case):
    """fqss_rowlin_bwd_w into a non-zero gw (split-K, fp32 atomics) through k_gemm_x3 and the fallback"""
    R, Ci, Co = case
    k = LIN_BWDW.index(case)
    x, _, _, gz = lin_operands(R, Ci, Co, 600 + k)
    ref, r32 = dw_ref(gz, x), gz.t() @ x
    start = torch.randn(Co, Ci, generator=gen(k)) * rms(ref)
    fails, tag = [], f"rowlin bwd_w {case}"
    for kind in kinds(k):
        fam = "x3" if kind == "x3" else "fb"
        measure(fam, "gw", lin_bwdw_run(gz, x, start, kind).double() - start.double(), ref, r32, f"{tag} {kind}", fails)
        if R > 32:
            kl = (R - 1) // 32 * 32
            floor(fam, "gw", dw_ref(gz[:kl], x[:kl]), ref, "last k-tile dropped", tag)
        if R > 1:
            floor(fam, "gw", dw_ref(gz[:R - 1], x[:R - 1]), ref, "last live row dropped", tag)
        floor(fam, "gw", dw_ref(torch.cat([gz, torch.full((1, Co), rms(gz))], 0), torch.cat([x, torch.full((1, Ci), rms(x))], 0)), ref,
              "row R read (values of the rms)", tag)
    h1, h2, _ = split3(gz)
    third_piece("x3", "gw", dw_ref(h1 + h2, x), ref, tag)
    assert not fails, fails


@gpu
def test_rowlin_exact_integers():
    """integer operands below 2^24 in the sum of the absolute products: all three forms, both implementations, bit for bit"""
    R, Ci, Co = 129, 70, 65
    g = gen(12)
    x, w, b, gz = ints(g, 200, R, Ci), ints(g, 100, Co, Ci), ints(g, 1000, Co), ints(g, 50, R, Co)
    start = ints(g, 1000, Co, Ci)
    assert exact_ok(x.double().abs() @ w.double().abs().t() + 1000, gz.double().abs() @ w.double().abs(),
                    gz.double().abs().t() @ x.double().abs() + 1000)
    for kind in ("x3", "odd", "off"):
        assert torch.equal(lin_fwd_run(x, w, b, kind, False), lin_ref(x, w, b).float()), kind
        assert torch.equal(lin_bwdx_run(gz, w, kind, False), dx_ref(gz, w).float()), kind
        assert torch.equal(lin_bwdw_run(gz, x, start, kind), (start.double() + dw_ref(gz, x)).float()), kind
    differs(lin_ref(x.roll(1, 1), w, b), lin_ref(x, w, b), "k index one off", "rowlin exact")


def planes_run(w):
    n = w.numel()
    wb = Vec(n, fill=w)
    pl = Cod(3, 2 * n)
    call("fqss_split3_planes", wb.ptr, pl.ptr, n, stream())
    assert wb.unchanged() and pl.written()
    return pl, pl.view.cpu().contiguous().view(torch.int16).reshape(3, n)


@gpu
@pytest.mark.parametrize("Ci", [32, 96, 256])
def test_rowlin_forward_presplit_weight(Ci):
    """fqss_split3_planes is exact (the three truncation pieces of the CPU split, <= 8 significant bits each, summing to w) and
    fqss_rowlin_fwd_w3 on those planes has the result bits of fqss_rowlin_fwd, over the three tile shapes"""
    for k, (R, Co) in enumerate([(129, 33), (64, 65), (127, 130)]):            # (2, 1), (1, 2), (2, 2)
        x, w, b, _ = lin_operands(R, Ci, Co, 700 + Ci + k)
        w = w * torch.exp(torch.randn(Co, Ci, generator=gen(k)) * 3)            # (pieces over a wide range of exponents)
        pl, bits = planes_run(w)
        want = torch.stack([(h.contiguous().view(torch.int32) >> 16).to(torch.int16) for h in split3(w)]).reshape(3, -1)
        assert torch.equal(bits, want), "fqss_split3_planes differs from the CPU split"
        back = (bits.to(torch.int32) << 16).view(torch.float32)
        assert torch.equal((back[0].double() + back[1].double() + back[2].double()).float(), w.reshape(-1))
        for bias in (b, None):
            assert torch.equal(lin_fwd_run(x, w, bias, "x3", k == 1, w3=pl), lin_fwd_run(x, w, bias, "x3", k == 1)), (R, Ci, Co)


@gpu
@pytest.mark.parametrize("kind", ["x3", "fallback"])
def test_rowlin_weight_gradient_batched(kind):
    """fqss_rowlin_bwd_w_batched: batch 2 with a negative sb_x and a gap between the gw slots, against float64 and against two single
    launches; "fallback": a batch stride with % 4 != 0 sends both problems to k_gemm_f32.  Nothing is written in the gap"""
    R, Ci, Co = 130, 68, 36
    ldg, ldx, ldw = 44, 72, 70
    sbg, sbx, sbw = R * ldg + 8, -(R * ldx + (5 if kind == "fallback" else 4)), Co * ldw + 12
    g = gen(21)
    gzs, xs = [heavy(g, R, Co) for _ in range(2)], [torch.randn(R, Ci, generator=g) for _ in range(2)]
    refs = [dw_ref(a, b) for a, b in zip(gzs, xs)]
    starts = [torch.randn(Co, Ci, generator=g) * rms(refs[0]) for _ in range(2)]
    gzf, xf = Flat(2 * sbg), Flat(2 * -sbx + 8)
    x0 = -sbx + 4                                                   # problem 0 sits BEHIND problem 1
    for p in range(2):
        gzf.put(p * sbg, gzs[p], ldg)
        xf.put(x0 + p * sbx, xs[p], ldx)
    gzf.snap()
    xf.snap()

    def gw_buffer():
        f = Flat(2 * sbw)
        for p in range(2):
            f.put(p * sbw, starts[p], ldw)
            f.mark(p * sbw, Co, Ci, ldw)
        f.snap()
        return f

    gw = gw_buffer()
    call("fqss_rowlin_bwd_w_batched", gzf.at(0), xf.at(x0), gw.at(0), R, Ci, Co, ldg, ldx, ldw, 2, sbg, sbx, sbw, stream())
    single = gw_buffer()
    for p in range(2):
        call("fqss_rowlin_bwd_w", gzf.at(p * sbg), xf.at(x0 + p * sbx), single.at(p * sbw), R, Ci, Co, ldg, ldx, ldw, stream())
    assert gzf.unchanged() and xf.unchanged() and gw.only_live_changed() and single.only_live_changed()
    fails, fam = [], ("x3" if kind == "x3" else "fb")
    for p in range(2):
        got, one = gw.cpu(p * sbw, Co, Ci, ldw).double() - starts[p].double(), single.cpu(p * sbw, Co, Ci, ldw).double() - starts[p].double()
        measure(fam, "gw", got, refs[p], gzs[p].t() @ xs[p], f"batched {kind} problem {p}", fails)
        measure(fam, "gw", got, one, None, f"batched {kind} problem {p} against its single launch", fails)
        floor(fam, "gw", dw_ref(gzs[p], xs[1 - p]), refs[p], "x of the other problem", f"batched {kind}")
    assert not fails, fails


@gpu
def test_rowlin_refusals():
    """each FQSS_REQUIRE of the float row entries; outputs untouched; R = 0 is a no-op"""
    R, Ci, Co = 5, 32, 8
    x, xo = [Blk(R, Ci, 36, off=o, fill=torch.zeros(R, Ci)) for o in (0, 1)]
    w, gz = Blk(Co, Ci, 36, fill=torch.zeros(Co, Ci)), Blk(R, Co, 12, fill=torch.zeros(R, Co))
    pl, plo = [Cod(3, 2 * Co * Ci, off=o, fill=torch.zeros(3, 2 * Co * Ci, dtype=torch.uint8)) for o in (0, 8)]
    z, gx, gw = Blk(R, Co, 12), Blk(R, Ci, 36), Blk(Co, Ci, 36)
    S, BIG = stream(), 1 << 31

    def fwd(x_=x.ptr, w_=w.ptr, z_=z.ptr, R=R, Ci=Ci, Co=Co, ldx=36, ldw=36, ldz=12):
        refused("fqss_rowlin_fwd", x_, w_, None, z_, R, Ci, Co, ldx, ldw, ldz, S)

    def fw3(x_=x.ptr, w_=pl.ptr, z_=z.ptr, R=R, Ci=Ci, Co=Co, ldx=36, ldz=12):
        refused("fqss_rowlin_fwd_w3", x_, w_, None, z_, R, Ci, Co, ldx, ldz, S)

    def bx(g_=gz.ptr, w_=w.ptr, gx_=gx.ptr, R=R, Ci=Ci, Co=Co, ldg=12, ldw=36, ldx=36):
        refused("fqss_rowlin_bwd_x", g_, w_, gx_, R, Ci, Co, ldg, ldw, ldx, S)

    def bw(g_=gz.ptr, x_=x.ptr, gw_=gw.ptr, R=R, Ci=Ci, Co=Co, ldg=12, ldx=36, ldw=36, batch=None):
        if batch is None:
            refused("fqss_rowlin_bwd_w", g_, x_, gw_, R, Ci, Co, ldg, ldx, ldw, S, who="rowlin_bwd_w")
        refused("fqss_rowlin_bwd_w_batched", g_, x_, gw_, R, Ci, Co, ldg, ldx, ldw, 1 if batch is None else batch, 0, 0, 0, S, who="rowlin_bwd_w")

    for f, names in ((fwd, ("x_", "w_", "z_")), (fw3, ("x_", "w_", "z_")), (bx, ("g_", "w_", "gx_")), (bw, ("g_", "x_", "gw_"))):
        for k in names:
            f(**{k: None})
        f(R=-1)
        f(R=BIG)
        f(Ci=0)
        f(Co=0)
    fwd(ldx=28)
    fwd(ldw=28)
    fwd(ldz=4)
    fw3(ldx=28)
    fw3(ldz=4)
    fw3(Ci=16, ldx=36)                   # Ci % 32
    fw3(w_=plo.ptr)                      # planes / activation rows not 16-B aligned
    fw3(x_=xo.ptr)
    fw3(ldx=38)
    bx(ldg=4)
    bx(ldw=28)
    bx(ldx=28)
    bw(ldg=4)
    bw(ldx=28)
    bw(ldw=28)
    bw(batch=0)
    bw(batch=65)
    assert z.untouched() and gx.untouched() and gw.untouched()
    call("fqss_rowlin_fwd", x.ptr, w.ptr, None, z.ptr, 0, Ci, Co, 36, 36, 12, S)
    call("fqss_rowlin_fwd_w3", x.ptr, pl.ptr, None, z.ptr, 0, Ci, Co, 36, 12, S)
    call("fqss_rowlin_bwd_x", gz.ptr, w.ptr, gx.ptr, 0, Ci, Co, 12, 36, 36, S)
    call("fqss_rowlin_bwd_w", gz.ptr, x.ptr, gw.ptr, 0, Ci, Co, 12, 36, 36, S)
    call("fqss_rowlin_bwd_w_batched", gz.ptr, x.ptr, gw.ptr, 0, Ci, Co, 12, 36, 36, 2, 0, 0, 0, S)
    assert z.untouched() and gx.untouched() and gw.untouched()


# ======================================================================================================= 6. coded gradient GEMMs
# (R, Ci, Co): k_gemm_x3<true, false, false, MI, NI, 2> with M = R, N = Ci, K = Co
QDX_CASES = [(1, 4, 4),               # (2, 1)
             (63, 20, 36),            # (2, 1); K = 32 + 4
             (64, 68, 32),            # (1, 2): M <= 64
             (65, 132, 80),           # (2, 2): 64 < M <= 128
             (257, 132, 256)]         # (1, 2): 3 x 2 tiles < 320
# (R, Ci, Co): k_gemm_x3<false, false, true, MI, NI, 1> with M = Co, N = Ci, K = R
QDW_CASES = [(1, 4, 4),               # (2, 1)
             (63, 64, 132),           # (2, 1), two row tiles, one k-slice
             (64, 132, 32),           # (1, 2)
             (65, 132, 132),          # (2, 2): four tiles, two slices
             (257, 68, 200),          # (2, 2): five slices
             (257, 260, 132)]         # (2, 2): three column tiles (the bias sums leave through the first one only)


def qdx_run(gz, wi, dw, zodd=False):
    R, Co = gz.shape
    Ci = wi.shape[1]
    gb, wc, dv = Blk(R, Co, Co + 8, fill=gz), Cod(Co, Ci, off=4, fill=wi), Vec(Co, fill=dw)
    gx = Blk(R, Ci, Ci + (5 if zodd else 4))
    call("fqss_qrow_bwd_x", gb.ptr, wc.ptr, dv.ptr, gx.ptr, R, Ci, Co, gb.ld, gx.ld, stream())
    all_unchanged(gz=gb, wi=wc, dw=dv)
    assert gx.written(), "fqss_qrow_bwd_x wrote outside [R][Ci]"
    return gx.cpu(R, Ci)


class QdwOps:
    def __init__(self, gz, c, lo, hi, k=0):
        (R, Co), Ci = gz.shape, c.shape[1]
        self.dims = (R, Ci, Co)
        self.gz = Blk(R, Co, Co + 4 + 4 * (k % 2), fill=gz)
        self.xc = Cod(R, Ci, Ci + 8 + 4 * (k % 3), off=4, fill=c)          # ld_xc > Ci, 4-B aligned only
        self.lo, self.hi = sc(lo), sc(hi)
        self.ld_gw = Ci + 3 + k % 2

    def unchanged(self):
        all_unchanged(gz=self.gz, xc=self.xc, lo=self.lo, hi=self.hi)

    def outputs(self, start, bstart):
        R, Ci, Co = self.dims
        return Blk(Co, Ci, self.ld_gw, fill=start), (Vec(Co, fill=bstart) if bstart is not None else None)

    def run(self, start, bstart=None):
        """fqss_qrow_bwd_w (bstart None) / fqss_qrow_bwd_wb -> gw, gbias on the CPU"""
        R, Ci, Co = self.dims
        gw, gb = self.outputs(start, bstart)
        h = [self.gz.ptr, self.xc.ptr, self.lo.ptr, self.hi.ptr, gw.ptr]
        if gb is None:
            call("fqss_qrow_bwd_w", *h, R, Ci, Co, self.gz.ld, self.xc.ld, gw.ld, stream())
        else:
            call("fqss_qrow_bwd_wb", *h, gb.ptr, R, Ci, Co, self.gz.ld, self.xc.ld, gw.ld, stream())
        self.unchanged()
        assert gw.written() and (gb is None or gb.written()), "the coded weight gradient wrote outside the Co x Ci of gw / the Co of gbias"
        return gw.cpu(Co, Ci), (gb.cpu() if gb is not None else None)

    def job(self, j, gw, gb):
        R, Ci, Co = self.dims
        j.gz, j.xc, j.qmin_x, j.qmax_x, j.gw, j.gbias = self.gz.ptr, self.xc.ptr, self.lo.ptr, self.hi.ptr, gw.ptr, ptr(gb)
        j.R, j.Ci, j.Co, j.ld_gz, j.ld_xc, j.ld_gw = R, Ci, Co, self.gz.ld, self.xc.ld, gw.ld


def group_run(opss, starts, bstarts):
    """one fqss_qrow_bwd_w_group call over the jobs -> [(gw, gbias | None)] on the CPU"""
    n = len(opss)
    arr = (_lib.FqssRowWgradJob * n)()
    outs = [o.outputs(s, b) for o, s, b in zip(opss, starts, bstarts)]
    for j, o, (gw, gb) in zip(arr, opss, outs):
        o.job(j, gw, gb)
    call("fqss_qrow_bwd_w_group", arr, n, stream())
    res = []
    for o, (gw, gb) in zip(opss, outs):
        o.unchanged()
        assert gw.written() and (gb is None or gb.written()), "fqss_qrow_bwd_w_group wrote outside a job's gw / gbias"
        res.append((gw.cpu(o.dims[2], o.dims[1]), gb.cpu() if gb is not None else None))
    return res


def qdx_pieces_operands(kind, seed):
    """gz = n 2^-20 whose split (after the scale by dw in {1, 2}) reaches the second ("two": |n| < 2^10) or third ("three": |n| < 2^17,
    weight codes in [-4, 3], K = Co = 8) bf16 piece"""
    g = gen(seed)
    if kind == "two":
        R, Ci, Co = 65, 36, 64
        wi, n = wcodes(g, Co, Ci), torch.randint(-1023, 1024, (R, Co), generator=g)
    else:
        R, Ci, Co = 63, 132, 8
        wi, n = wcodes(g, Co, Ci, lim=4), torch.randint(-(2 ** 17) + 1, 2 ** 17, (R, Co), generator=g)
    dw = torch.where(torch.arange(Co) % 2 == 0, 1.0, 2.0)
    return wi, n, n.float() * 2.0 ** -20, dw


@gpu
def test_coded_dgrad_exact_integers():
    """fqss_qrow_bwd_x with dw in {1, 2, 4} and integer gz: the integer sum bit for bit over every tile shape"""
    for k, (R, Ci, Co) in enumerate(QDX_CASES):
        g = gen(800 + k)
        wi, gz, dw = wcodes(g, Co, Ci), ints(g, 8, R, Co), 2.0 ** torch.randint(0, 3, (Co,), generator=g).float()
        assert exact_ok((gz.double().abs() * dw.double()) @ wi.double().abs())
        ref = qdx_ref(gz, wi, dw)
        assert torch.equal(qdx_run(gz, wi, dw, zodd=k % 2 == 1), ref.float()), (R, Ci, Co)
        if Co > 1:
            differs(qdx_ref(gz, wi.roll(1, 0), dw), ref, "reduction row one off", f"coded dgrad exact {(R, Ci, Co)}")
            differs(qdx_ref(gz, wi, dw.roll(1)), ref, "dw of the neighbouring row", f"coded dgrad exact {(R, Ci, Co)}")


@gpu
@pytest.mark.parametrize("kind", ["two", "three"])
def test_coded_dgrad_exact_through_the_bf16_pieces(kind):
    """gz = n 2^-20 with more than 8 (16) significant bits, dw a power of two: every partial sum is an exact multiple of 2^-20 below
    2^24 of them -- bit-equal, and a kernel without the piece is not"""
    wi, n, gz, dw = qdx_pieces_operands(kind, 7)
    h1, h2, h3 = split3(gz * dw)
    assert bool((h2 != 0).any()) and (kind == "two" or bool((h3 != 0).any()))
    assert exact_ok((n.double().abs() * dw.double()) @ wi.double().abs())
    ref = qdx_ref(gz, wi, dw)
    assert torch.equal(qdx_run(gz, wi, dw), ref.float()), kind
    differs((h1 + h2 if kind == "three" else h1).double() @ wi.double(), ref, f"bf16 piece {3 if kind == 'three' else 2} of gz dropped",
            f"coded dgrad pieces {kind}")


@gpu
@pytest.mark.parametrize("case", QDX_CASES, ids=str)
def test_coded_dgrad_against_fp64(case):
    """fqss_qrow_bwd_x with heavy-tailed gz and real steps, ld_gz > Co, ld_gx > Ci, weight codes 4-B aligned only"""
    R, Ci, Co = case
    k = QDX_CASES.index(case)
    g = gen(850 + k)
    wi, dw, gz = wcodes(g, Co, Ci), steps(g, Co), heavy(g, R, Co)
    ref, r32 = qdx_ref(gz, wi, dw), gz @ (wi.float() * dw[:, None])
    fails, tag = [], f"coded dgrad {case}"
    measure("qdx", "gx", qdx_run(gz, wi, dw, zodd=k % 2 == 0), ref, r32, tag, fails)
    assert not fails, fails
    kl = (Co - 1) // 32 * 32 if Co > 32 else Co - min(4, Co - 1)
    floor("qdx", "gx", qdx_ref(gz[:, :kl], wi[:kl], dw[:kl]), ref, "last k-tile (K <= 32: the last four k) dropped", tag)
    floor("qdx", "gx", qdx_ref(gz, wi, dw.roll(1)), ref, "dw of the neighbouring row", tag)
    floor("qdx", "gx", qdx_ref(gz, wi.roll(1, 1), dw), ref, "last live column dropped for its neighbour", tag)
    floor("qdx", "gx", qdx_ref(torch.cat([gz, torch.full((R, 1), rms(gz))], 1), torch.cat([wi, torch.full((1, Ci), 74, dtype=torch.int8)], 0),
                               torch.cat([dw, dw[:1]])), ref, "padding column Co of gz read (a gz of the rms against codes of their rms)", tag)
    h1, h2, _ = split3(gz * dw)
    third_piece("qdx", "gx", (h1 + h2).double() @ wi.double(), ref, tag)


def qdw_exact_operands(R, Ci, Co, seed):
    g = gen(seed)
    return ints(g, 8, R, Co), codes(g, R, Ci), ints(g, 1000, Co, Ci), ints(g, 1000, Co)


@gpu
def test_coded_wgrad_exact_integers():
    """fqss_qrow_bwd_w, _wb and the group with integer gz, dx = 1 and min_x = -3: gw and gbias are the integer sums bit for bit, whatever
    order the atomics arrive in"""
    opss, starts, bstarts, refs = [], [], [], []
    for k, (R, Ci, Co) in enumerate(QDW_CASES):
        gz, c, start, bstart = qdw_exact_operands(R, Ci, Co, 900 + k)
        assert exact_ok(gz.double().abs().t() @ (c.double() + 3) + start.abs(), gz.double().abs().sum(0) + bstart.abs())
        ref, bref = (start.double() + qdw_ref(gz, c, -3.0, 252.0)).float(), (bstart.double() + gz.double().sum(0)).float()
        ops = QdwOps(gz, c, -3.0, 252.0, k)
        assert torch.equal(ops.run(start)[0], ref), (R, Ci, Co)
        gw, gb = ops.run(start, bstart)
        assert torch.equal(gw, ref) and torch.equal(gb, bref), (R, Ci, Co)
        tag = f"coded wgrad exact {(R, Ci, Co)}"
        differs(start.double() + qdw_ref(gz, c, -3.0, 252.0, dropmin=True), ref, "min_x rowsum dropped", tag)
        if R > 1:
            differs(start.double() + qdw_ref(gz[:R - 1], c[:R - 1], -3.0, 252.0), ref, "last live row dropped", tag)
        if Ci > 128:
            differs(bstart.double() + 2 * gz.double().sum(0), bref, "gbias added once per column tile", tag)
        opss.append(ops), starts.append(start), bstarts.append(bstart if k % 2 else None), refs.append((ref, bref))
    for k, ((gw, gb), (ref, bref)) in enumerate(zip(group_run(opss, starts, bstarts), refs)):
        assert torch.equal(gw, ref) and (gb is None or torch.equal(gb, bref)), QDW_CASES[k]


def qdw_pieces_operands(seed=17):
    """gz = n 2^-20 with |n| < 2^17 (all three bf16 pieces) against codes 0 .. 3 at R = 33, start an integer number of 2^-20"""
    R, Ci, Co = 33, 132, 68
    g = gen(seed)
    n = torch.randint(-(2 ** 17) + 1, 2 ** 17, (R, Co), generator=g)
    c = torch.randint(0, 4, (R, Ci), generator=g, dtype=torch.uint8)
    return n, n.float() * 2.0 ** -20, c, ints(g, 1000, Co, Ci) * 2.0 ** -20, ints(g, 1000, Co) * 2.0 ** -20


@gpu
def test_coded_wgrad_exact_through_the_bf16_pieces():
    """every partial sum of gw and of the row sums is an exact multiple of 2^-20 below 2^24 of them (dx = 1, min_x = -3): the three
    entries are bit-equal -- and a kernel without the third piece is not"""
    n, gz, c, start, bstart = qdw_pieces_operands()
    h1, h2, h3 = split3(gz)
    assert bool((h2 != 0).any()) and bool((h3 != 0).any())
    assert exact_ok(n.double().abs().t() @ (c.double() + 3) + 1000, 3 * n.double().abs().sum(0) + 1000)
    ref, bref = (start.double() + qdw_ref(gz, c, -3.0, 252.0)).float(), (bstart.double() + gz.double().sum(0)).float()
    ops = QdwOps(gz, c, -3.0, 252.0)
    assert torch.equal(ops.run(start)[0], ref)
    gw, gb = ops.run(start, bstart)
    assert torch.equal(gw, ref) and torch.equal(gb, bref)
    (gw, gb), = group_run([ops], [start], [bstart])
    assert torch.equal(gw, ref) and torch.equal(gb, bref)
    differs(start.double() + qdw_ref(h1 + h2, c, -3.0, 252.0), ref, "bf16 piece 3 of gz dropped", "coded wgrad pieces")
    differs(start.double() + qdw_ref(h1, c, -3.0, 252.0), start.double() + qdw_ref(h1 + h2, c, -3.0, 252.0), "bf16 piece 2 of gz dropped", "coded wgrad pieces")


def qdw_real_operands(R, Ci, Co, seed):
    g = gen(seed)
    return heavy(g, R, Co), codes(g, R, Ci), -1.3, 2.1


def qdw_floors(fam, gz, c, lo, hi, ref, tag):
    R = gz.shape[0]
    if R > 32:
        kl = (R - 1) // 32 * 32
        floor(fam, "gw", qdw_ref(gz[:kl], c[:kl], lo, hi), ref, "last k-tile dropped", tag)
    floor(fam, "gw", qdw_ref(gz, c, lo, hi, dropmin=True), ref, "min_x rowsum dropped", tag)
    if R > 1:
        floor(fam, "gw", qdw_ref(gz[:R - 1], c[:R - 1], lo, hi), ref, "last live row dropped", tag)
        floor(fam, "gb", gz[:R - 1].double().sum(0), gz.double().sum(0), "last live row dropped", tag)
    one, c255 = torch.full_like(gz[:1], rms(gz)), torch.full_like(c[:1], 255)
    floor(fam, "gw", qdw_ref(torch.cat([gz, one], 0), torch.cat([c, c255], 0), lo, hi), ref, "row R read (gz of the rms, code 255)", tag)
    h1, h2, _ = split3(gz)
    third_piece(fam, "gw", qdw_ref(h1 + h2, c, lo, hi), ref, tag)


@gpu
@pytest.mark.parametrize("case", QDW_CASES, ids=str)
def test_coded_wgrad_against_fp64(case):
    """fqss_qrow_bwd_w and fqss_qrow_bwd_wb with heavy-tailed gz, range [-1.3, 2.1], ld_xc > Ci, ld_gw > Ci, non-zero starts: gw of the
    two entries bit-identical where one k-slice adds (R <= 64), gbias = start + the column sums, added once"""
    R, Ci, Co = case
    k = QDW_CASES.index(case)
    gz, c, lo, hi = qdw_real_operands(R, Ci, Co, 950 + k)
    ref, bref = qdw_ref(gz, c, lo, hi), gz.double().sum(0)
    start, bstart = torch.randn(Co, Ci, generator=gen(k)) * rms(ref), torch.randn(Co, generator=gen(k)) * rms(bref)
    r32 = gz.t() @ (delta32(lo, hi) * c.float() + f32(lo))
    ops = QdwOps(gz, c, lo, hi, k)
    fails, tag = [], f"coded wgrad {case}"
    gw, _ = ops.run(start)
    gwb, gb = ops.run(start, bstart)
    measure("qdw", "gw", gw.double() - start.double(), ref, r32, tag, fails)
    measure("qdw", "gw", gwb.double() - start.double(), ref, r32, tag + " _wb", fails)
    measure("qdw", "gb", gb.double() - bstart.double(), bref, gz.sum(0), tag + " _wb", fails)
    assert not fails, fails
    if R <= 64:
        assert torch.equal(gw, gwb), "one k-slice: fqss_qrow_bwd_wb's gw differs from fqss_qrow_bwd_w"
    if R > 1 and Ci > 128:
        floor("qdw", "gb", 2 * bref, bref, "gbias added once per column tile", tag)
    qdw_floors("qdw", gz, c, lo, hi, ref, tag)


@gpu
def test_coded_wgrad_batched():
    """fqss_qrow_bwd_w_batched: two column blocks of one gz against one code image (sb_xc = 0), a gap between the gw slots"""
    R, Ci, Co = 130, 68, 36
    g = gen(33)
    gz, c, lo, hi = heavy(g, R, 2 * Co), codes(g, R, Ci), -1.3, 2.1
    refs = [qdw_ref(gz[:, p * Co:(p + 1) * Co], c, lo, hi) for p in range(2)]
    starts = [torch.randn(Co, Ci, generator=g) * rms(refs[0]) for _ in range(2)]
    gb, xc, lov, hiv = Blk(R, 2 * Co, 2 * Co + 8, fill=gz), Cod(R, Ci, Ci + 12, off=4, fill=c), sc(lo), sc(hi)
    ldw, sbw = Ci + 2, Co * (Ci + 2) + 10
    gw = Flat(2 * sbw)
    for p in range(2):
        gw.put(p * sbw, starts[p], ldw)
        gw.mark(p * sbw, Co, Ci, ldw)
    gw.snap()
    call("fqss_qrow_bwd_w_batched", gb.ptr, xc.ptr, lov.ptr, hiv.ptr, gw.at(0), R, Ci, Co, gb.ld, xc.ld, ldw, 2, Co, 0, sbw, stream())
    all_unchanged(gz=gb, xc=xc, lo=lov, hi=hiv)
    assert gw.only_live_changed(), "a write beside the two gw slots"
    fails = []
    for p in range(2):
        got = gw.cpu(p * sbw, Co, Ci, ldw)
        assert bool(torch.isfinite(got).all())
        measure("qdw", "gw", got.double() - starts[p].double(), refs[p], None, f"coded wgrad batched problem {p}", fails)
        floor("qdw", "gw", refs[1 - p], refs[p], "the other column block", "coded wgrad batched")
    assert not fails, fails


# (R, Ci, Co) of the group's jobs: 34 jobs of the (2, 1) shape (Ci <= 64: two launches of k_gemm_x3_wq_multi<2, 1>), (1, 2) (Ci > 64, Co <= 64)
# and (2, 2) jobs beside them, R over {255, 256, 257, 600} (kchunk >= 256: one, one, two and three k-slices) and one single-row job
GROUP_JOBS = [((255, 256, 257, 600)[k % 4], (20, 64, 36, 4)[k % 4], (12, 132, 68, 36)[k % 3]) for k in range(34)] + \
             [(255, 132, 32), (600, 68, 64), (256, 132, 68), (257, 260, 132), (600, 132, 200), (1, 68, 4)]


def group_operands():
    opss, starts, bstarts, refs = [], [], [], []
    for k, (R, Ci, Co) in enumerate(GROUP_JOBS):
        gz, c, lo, hi = qdw_real_operands(R, Ci, Co, 1000 + k)
        lo, hi = lo - 0.1 * (k % 3), hi + 0.2 * (k % 2)
        ref, bref = qdw_ref(gz, c, lo, hi), gz.double().sum(0)
        refs.append((ref, bref, gz, c, lo, hi))
        starts.append(torch.randn(Co, Ci, generator=gen(k)) * rms(ref))
        bstarts.append(torch.randn(Co, generator=gen(k)) * rms(bref) if k % 2 == 0 else None)
        opss.append(QdwOps(gz, c, lo, hi, k))
    return opss, starts, bstarts, refs


@gpu
def test_coded_wgrad_group():
    """fqss_qrow_bwd_w_group over 40 jobs of the three tile shapes, gbias null and non-null mixed: each job against float64; the whole
    call repeated on re-initialised outputs -- bit-identical for the jobs of one k-slice (R <= 256: one add per element).  Jobs of
    several slices add with fp32 atomics in the order the workgroups retire: no run-to-run assertion there (see the docstring)"""
    opss, starts, bstarts, refs = group_operands()
    run1, run2 = group_run(opss, starts, bstarts), group_run(opss, starts, bstarts)
    fails = []
    for k, ((gw, gb), (gw2, gb2), (ref, bref, gz, c, lo, hi)) in enumerate(zip(run1, run2, refs)):
        tag = f"group job {k} {GROUP_JOBS[k]}"
        if GROUP_JOBS[k][0] <= 256:
            assert torch.equal(gw, gw2) and (gb is None or torch.equal(gb, gb2)), (tag, "not reproducible")
        measure("group", "gw", gw.double() - starts[k].double(), ref, None, tag, fails)
        if gb is not None:
            measure("group", "gb", gb.double() - bstarts[k].double(), bref, None, tag, fails)
        if k >= 30:
            qdw_floors("group", gz, c, lo, hi, ref, tag)
    assert not fails, fails


@gpu
def test_coded_gradient_refusals():
    """each FQSS_REQUIRE of fqss_qrow_bwd_x, fqss_qrow_bwd_w / _wb / _batched and fqss_qrow_bwd_w_group; outputs untouched; R = 0 and
    njobs = 0 are no-ops"""
    R, Ci, Co = 5, 32, 8
    gz, go = [Blk(R, Co, 12, off=o, fill=torch.zeros(R, Co)) for o in (0, 1)]
    wi, wo = [Cod(Co, Ci, off=o, fill=torch.zeros(Co, Ci, dtype=torch.int8)) for o in (0, 2)]
    xc, xo = [Cod(R, Ci, 36, off=o, fill=torch.zeros(R, Ci, dtype=torch.uint8)) for o in (0, 2)]
    dw, dwo = Vec(Co, fill=1.0), Blk(1, Co, Co, off=1, fill=torch.ones(1, Co))
    lo, hi = sc(0.0), sc(255.0)
    gx, gw, gb = Blk(R, Ci, 36), Blk(Co, Ci, 36), Vec(Co)
    S, BIG = stream(), 1 << 31

    def bx(g_=gz.ptr, w_=wi.ptr, d_=dw.ptr, gx_=gx.ptr, R=R, Ci=Ci, Co=Co, ldg=12, ldx=36):
        refused("fqss_qrow_bwd_x", g_, w_, d_, gx_, R, Ci, Co, ldg, ldx, S)

    def bw(g_=gz.ptr, x_=xc.ptr, lo_=lo.ptr, hi_=hi.ptr, gw_=gw.ptr, R=R, Ci=Ci, Co=Co, ldg=12, ldx=36, ldw=36):
        refused("fqss_qrow_bwd_w", g_, x_, lo_, hi_, gw_, R, Ci, Co, ldg, ldx, ldw, S, who="qrow_bwd_w")
        refused("fqss_qrow_bwd_wb", g_, x_, lo_, hi_, gw_, gb.ptr, R, Ci, Co, ldg, ldx, ldw, S, who="qrow_bwd_w")
        refused("fqss_qrow_bwd_w_batched", g_, x_, lo_, hi_, gw_, R, Ci, Co, ldg, ldx, ldw, 1, 0, 0, 0, S, who="qrow_bwd_w")
        j = (_lib.FqssRowWgradJob * 2)()                                         # the group: a good job in front of the bad one
        j[0].gz, j[0].xc, j[0].qmin_x, j[0].qmax_x, j[0].gw, j[0].gbias = gz.ptr, xc.ptr, lo.ptr, hi.ptr, gw.ptr, gb.ptr
        j[0].R, j[0].Ci, j[0].Co, j[0].ld_gz, j[0].ld_xc, j[0].ld_gw = 5, 32, 8, 12, 36, 36
        j[1].gz, j[1].xc, j[1].qmin_x, j[1].qmax_x, j[1].gw, j[1].gbias = g_, x_, lo_, hi_, gw_, None
        j[1].R, j[1].Ci, j[1].Co, j[1].ld_gz, j[1].ld_xc, j[1].ld_gw = R, Ci, Co, ldg, ldx, ldw
        refused("fqss_qrow_bwd_w_group", j, 2, S)

    def bwb(batch=2, sbg=0, sbx=0):
        refused("fqss_qrow_bwd_w_batched", gz.ptr, xc.ptr, lo.ptr, hi.ptr, gw.ptr, R, Ci, Co, 12, 36, 36, batch, sbg, sbx, 0, S, who="qrow_bwd_w")

    for k in ("g_", "w_", "d_", "gx_"):
        bx(**{k: None})
    bx(R=-1)
    bx(R=BIG)
    bx(Ci=0)
    bx(Co=0)
    bx(ldg=4)
    bx(ldx=28)
    bx(Ci=30)                            # Ci % 4, Co % 4, ld_gz % 4, alignment of gz / wi / dw
    bx(Co=6)
    bx(ldg=14)
    bx(g_=go.ptr)
    bx(w_=wo.ptr)
    bx(d_=dwo.ptr)
    for k in ("g_", "x_", "lo_", "hi_", "gw_"):
        bw(**{k: None})
    bw(R=-1)
    bw(R=BIG)
    bw(Ci=0)
    bw(Co=0)
    bw(ldg=4)
    bw(ldx=28)
    bw(ldw=28)
    bw(Ci=30)
    bw(Co=6)
    bw(ldg=14)
    bw(ldx=38)
    bw(g_=go.ptr)
    bw(x_=xo.ptr)
    refused("fqss_qrow_bwd_wb", gz.ptr, xc.ptr, lo.ptr, hi.ptr, gw.ptr, None, R, Ci, Co, 12, 36, 36, S)       # null bias gradient
    bwb(batch=0)
    bwb(batch=65)
    bwb(sbg=6)
    bwb(sbx=6)
    # the group: no job array, R = 0 in a job (the flat entries take it as a no-op), more than 1024 jobs
    j = (_lib.FqssRowWgradJob * 1025)()
    for q in range(1025):
        j[q].gz, j[q].xc, j[q].qmin_x, j[q].qmax_x, j[q].gw, j[q].gbias = gz.ptr, xc.ptr, lo.ptr, hi.ptr, gw.ptr, gb.ptr
        j[q].R, j[q].Ci, j[q].Co, j[q].ld_gz, j[q].ld_xc, j[q].ld_gw = R, Ci, Co, 12, 36, 36
    refused("fqss_qrow_bwd_w_group", j, 1025, S)
    refused("fqss_qrow_bwd_w_group", None, 1, S)
    refused("fqss_qrow_bwd_w_group", j, -1, S)
    j[1].R = 0
    refused("fqss_qrow_bwd_w_group", j, 2, S)
    assert gx.untouched() and gw.untouched() and gb.untouched()
    call("fqss_qrow_bwd_x", gz.ptr, wi.ptr, dw.ptr, gx.ptr, 0, Ci, Co, 12, 36, S)
    call("fqss_qrow_bwd_w", gz.ptr, xc.ptr, lo.ptr, hi.ptr, gw.ptr, 0, Ci, Co, 12, 36, 36, S)
    call("fqss_qrow_bwd_wb", gz.ptr, xc.ptr, lo.ptr, hi.ptr, gw.ptr, gb.ptr, 0, Ci, Co, 12, 36, 36, S)
    call("fqss_qrow_bwd_w_batched", gz.ptr, xc.ptr, lo.ptr, hi.ptr, gw.ptr, 0, Ci, Co, 12, 36, 36, 2, 0, 0, 0, S)
    call("fqss_qrow_bwd_w_group", j, 0, S)
    call("fqss_qrow_bwd_w_group", None, 0, S)
    assert gx.untouched() and gw.untouched() and gb.untouched()


# ============================================================================================================ 7. deterministic mode
@pytest.fixture
def det_off():
    yield
    if K is not None:
        K.DetMode.off()          # (the control block is device-wide: no later test may run under it)


@gpu
def test_row_weight_gradients_deterministic_mode(det_off):
    """FQSS_DETERMINISTIC=1 arithmetic of the row weight gradients' atomics (integer sums on the shadow of the attached slot-0 arena,
    fqss_det_finish rounds once): fqss_rowlin_bwd_w, fqss_qrow_bwd_wb and fqss_qrow_bwd_w_group into slices of the arena, twice each --
    bit-identical, within the family's bound, nothing beside the slots"""
    R, Ci, Co = 1030, 132, 68
    g = gen(41)
    x, gzf = torch.randn(R, Ci, generator=g), heavy(g, R, Co)
    xb, gfb = Blk(R, Ci, Ci + 4, fill=x), Blk(R, Co, Co + 8, fill=gzf)
    jobs = [(600, 132, 68), (257, 36, 12), (600, 68, 32)]
    qd = [qdw_real_operands(r, ci, co, 60 + k) for k, (r, ci, co) in enumerate([(R, Ci, Co)] + jobs)]
    qops = [QdwOps(gz, c, lo, hi, k) for k, (gz, c, lo, hi) in enumerate(qd)]
    # slots of the arena: (name, offset, rows, columns, float64 reference, family, tensor)
    slots, off = [], 64
    for name, ref, fam, ten in [("rowlin", dw_ref(gzf, x), "x3", "gw"), ("wb gw", qdw_ref(*qd[0]), "qdw", "gw"),
                                ("wb gb", qd[0][0].double().sum(0)[None], "qdw", "gb")] + \
            [(f"group {k} gw", qdw_ref(*qd[k + 1]), "group", "gw") for k in range(3)] + \
            [(f"group {k} gb", qd[k + 1][0].double().sum(0)[None], "group", "gb") for k in (0, 2)]:
        slots.append((name, off, ref, fam, ten, torch.randn(ref.shape, generator=g) * rms(ref)))
        off += (ref.numel() + 63) // 64 * 64 + 64
    at = {s[0]: s[1] for s in slots}
    arena = torch.zeros(off, device=DEV)
    p = lambda name: arena.data_ptr() + 4 * at[name]
    det = K.DetMode()
    det.attach(0, arena)
    det.activate()
    runs = []
    for _ in range(2):
        arena.zero_()
        for name, o, ref, fam, ten, start in slots:
            arena[o:o + ref.numel()].copy_(start.reshape(-1))
        call("fqss_rowlin_bwd_w", gfb.ptr, xb.ptr, p("rowlin"), R, Ci, Co, gfb.ld, xb.ld, Ci, stream())
        q = qops[0]
        call("fqss_qrow_bwd_wb", q.gz.ptr, q.xc.ptr, q.lo.ptr, q.hi.ptr, p("wb gw"), p("wb gb"), R, Ci, Co, q.gz.ld, q.xc.ld, Ci, stream())
        arr = (_lib.FqssRowWgradJob * 3)()
        for k, (r, ci, co) in enumerate(jobs):
            q, j = qops[k + 1], arr[k]
            j.gz, j.xc, j.qmin_x, j.qmax_x, j.gw, j.gbias = q.gz.ptr, q.xc.ptr, q.lo.ptr, q.hi.ptr, p(f"group {k} gw"), (p(f"group {k} gb") if k != 1 else None)
            j.R, j.Ci, j.Co, j.ld_gz, j.ld_xc, j.ld_gw = r, ci, co, q.gz.ld, q.xc.ld, ci
        call("fqss_qrow_bwd_w_group", arr, 3, stream())
        det.finish(0)
        torch.cuda.synchronize()
        runs.append(arena.cpu().clone())
    K.DetMode.off()
    all_unchanged(x=xb, gz=gfb)
    for q in qops:
        q.unchanged()
    assert torch.equal(runs[0], runs[1]), "deterministic mode: the sums of two runs differ"
    a, beside, fails = runs[0], torch.ones(off, dtype=torch.bool), []
    for name, o, ref, fam, ten, start in slots:
        beside[o:o + ref.numel()] = False
        measure(fam, ten, a[o:o + ref.numel()].reshape(ref.shape).double() - start.double(), ref, None, f"deterministic {name}", fails)
    assert bool((a[beside] == 0).all()), "a write beside the gradient slots"
    assert not fails, fails


# ==================================================================================================== the references, without a GPU
def test_references_on_cpu():
    """the float64 references of this file equal float64 F.linear on oracle weight_quantize / act_quantize operands and that graph's
    autograd; the exact-integer constructions stay below 2^24; the piece cases have their pieces; the range shares of the fused-quantizer
    cases hold on the reference z; every value of every axis the issue names is in the grids"""
    g = gen(3)
    R, Ci, Co = 65, 48, 33
    w = (torch.randn(Co, Ci, generator=g) * 0.05).double()
    a = (127.5 * 2.0 ** -9 * (1 + torch.arange(Co) % 3)).double()[:, None]
    xlo, xhi = torch.tensor([-0.75], dtype=F64), torch.tensor([-0.75 + 255 * 2.0 ** -7], dtype=F64)
    x = (torch.randn(R, Ci, generator=g) * 0.8 + 0.4).double()
    b = torch.randn(Co, generator=g).double()
    wi, c = O.weight_indices(w, -a, a), O.act_indices(x, xlo, xhi)
    dw = (2 * a / 255)[:, 0].float()
    assert torch.equal(dw.double(), (2 * a / 255)[:, 0]) and float(delta32(float(xlo), float(xhi))) == 2.0 ** -7
    wq, xq = O.weight_quantize(w, -a, a).requires_grad_(), O.act_quantize(x, xlo, xhi).requires_grad_()
    z = F.linear(xq, wq, b)
    assert errs(z.detach(), qfwd_ref(wi, c, dw, b, float(xlo), float(xhi)))[0] <= 1e-12
    gz = heavy(g, R, Co)
    z.backward(gz.double())
    assert errs(xq.grad, qdx_ref(gz, wi, dw))[0] <= 1e-12
    assert errs(wq.grad, qdw_ref(gz, c, float(xlo), float(xhi)))[0] <= 1e-12
    xf, wf = x.clone().requires_grad_(), w.clone().requires_grad_()
    zf = F.linear(xf, wf, b)
    zf.backward(gz.double())
    assert errs(zf.detach(), lin_ref(x, w, b))[0] <= 1e-12 and errs(xf.grad, dx_ref(gz, w))[0] <= 1e-12 and errs(wf.grad, dw_ref(gz, x))[0] <= 1e-12
    # the derived bound carries the cancelling terms: mag >= |ref| and >= |dw dx S'|
    Sp, Rk, t1, t2, t3, mag = qfwd_parts(wi, c, dw, b, float(xlo), float(xhi))
    assert bool((mag >= (t1 + t2 + t3).abs() * (1 - 1e-12)).all()) and bool((mag >= (dw.double() * 2.0 ** -7 * Sp).abs() * (1 - 1e-12)).all())
    # split3 is exact, and the second / third pieces of the piece cases are there
    h1, h2, h3 = split3(gz)
    assert torch.equal((h1.double() + h2.double() + h3.double()).float(), gz) and bool((h3 != 0).any())
    for kind in ("two", "three"):
        wik, n, gzk, dwk = qdx_pieces_operands(kind, 7)
        p1, p2, p3 = split3(gzk * dwk)
        assert exact_ok((n.double().abs() * dwk.double()) @ wik.double().abs()) and bool((p2 != 0).any()) and (kind == "two" or bool((p3 != 0).any()))
        assert torch.equal(p1 + p2 + p3, gzk * dwk) and (kind == "three" or bool((p3 == 0).all()))
    n, gzk, ck, st, bst = qdw_pieces_operands()
    p1, p2, p3 = split3(gzk)
    assert bool((p2 != 0).any()) and bool((p3 != 0).any()) and exact_ok(n.double().abs().t() @ (ck.double() + 3) + 1000, 3 * n.double().abs().sum(0) + 1000)
    # the exact-integer constructions
    for k, case in enumerate(QROW_CASES):
        wi_, c_, dw_, b_, lo_, hi_ = qrow_operands(*case[:3], case[5], "min" if k % 2 else "int", 100 + k)
        assert float(delta32(lo_, hi_)) == 1.0 and qrow_exact_ok(wi_, c_, b_, lo_), case
    for k, case in enumerate([(129, 1024, 130, 16, "st", True), (33, 1024, 65, 0, "odd", False), (31, 80, 3, 48, "st", True)]):
        wi_, c_, dw_, b_, lo_, hi_ = qrow_operands(*case[:3], case[5], "ext", 150 + k)
        assert qrow_exact_ok(wi_, c_, b_, lo_) and set(wi_.unique().tolist()) == {-128, 127} and set(c_.unique().tolist()) == {0, 255}, case
    for k, (Rc, Cic, Coc) in enumerate(QDX_CASES):
        gk = gen(800 + k)
        wi_, gz_, dw_ = wcodes(gk, Coc, Cic), ints(gk, 8, Rc, Coc), 2.0 ** torch.randint(0, 3, (Coc,), generator=gk).float()
        assert exact_ok((gz_.double().abs() * dw_.double()) @ wi_.double().abs()), (Rc, Cic, Coc)
    for k, (Rc, Cic, Coc) in enumerate(QDW_CASES):
        gz_, c_, st_, bst_ = qdw_exact_operands(Rc, Cic, Coc, 900 + k)
        assert exact_ok(gz_.double().abs().t() @ (c_.double() + 3) + st_.abs(), gz_.double().abs().sum(0) + bst_.abs()), (Rc, Cic, Coc)
    # a visible share of z below, inside and above each range of the fused-quantizer cases
    for k, (Rc, Cic, Coc, act, lz, ly) in enumerate(FWDQ_CASES):
        wi_, c_, dw_, b_, lo_, hi_ = qrow_operands(Rc, Cic, Coc, True, "real", 300 + k)
        rng, t = fwdq_ranges(qfwd_ref(wi_, c_, dw_, b_, lo_, hi_), act)
        assert min(shares(t, rng)) > 0.1 and (act != ACT_POST_RELU or rng[0] < 0 < rng[1]), (k, shares(t, rng), rng)
    for (Rc, Cic, Coc) in FWDQ2_CASES:
        wi_, c_, dw_, b_, lo_, hi_ = qrow_operands(Rc, Cic, Coc, True, "real", 350 + Cic)
        zr = qfwd_ref(wi_, c_, dw_, b_, lo_, hi_)
        r1, r2, t = fwdq2_ranges(zr)
        assert r1[0] < 0 < r1[1] and min(shares(zr.float(), r1)) > 0.1 and min(shares(t, r2)) > 0.1, (Cic, shares(zr.float(), r1), shares(t, r2))
    # every value of every axis the issue names is in the grids
    ax = lambda cases, k: {c[k] for c in cases}
    assert ax(QROW_CASES, 0) == {1, 31, 33, 127, 128, 129, 257} and ax(QROW_CASES, 1) == {16, 32, 48, 64, 80, 256, 1024, 2048}
    assert ax(QROW_CASES, 2) == {1, 3, 33, 64, 65, 96, 130, 192} and ax(QROW_CASES, 3) == {0, 16, 48} and ax(QROW_CASES, 4) == {"st", "odd", "off"}
    assert ax(QROW_CASES, 5) == {True, False} and any(64 < c[2] <= 96 and c[4] == "st" for c in QROW_CASES)
    assert any(c[2] % 4 and c[2] > 64 and c[4] == "st" for c in QROW_CASES) and {c[3] for c in FWDQ_CASES} == {ACT_NONE, ACT_RELU, ACT_PRELU, ACT_POST_RELU}
    assert set(LIN_FWD) >= {(1, 4, 1), (33, 20, 3), (129, 48, 33), (64, 32, 65), (127, 80, 130), (300, 256, 130), (41000, 32, 130)}
    assert set(LIN_BWDX) >= {(129, 33, 48), (64, 65, 32), (127, 130, 80), (300, 130, 256), (33000, 130, 32)}
    assert ax(LIN_BWDW, 0) == {1, 63, 65, 130, 257, 1030, 4200} and (4200, 256, 256) in LIN_BWDW
    assert {(c[1], c[2]) for c in LIN_BWDW} == {(4, 1), (20, 33), (64, 130), (130, 33), (130, 130), (65, 200), (256, 256)}
    assert ax(QDX_CASES, 0) == ax(QDW_CASES, 0) == {1, 63, 64, 65, 257} and ax(GROUP_JOBS, 0) == {1, 255, 256, 257, 600}
    tile = lambda Cic, Coc: (2, 1) if Cic <= 64 else ((1, 2) if Coc <= 64 else (2, 2))
    count = {t: sum(tile(j[1], j[2]) == t for j in GROUP_JOBS) for t in ((2, 1), (1, 2), (2, 2))}
    assert count[(2, 1)] > 32 and count[(1, 2)] >= 2 and count[(2, 2)] >= 3, count
