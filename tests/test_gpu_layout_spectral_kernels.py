"""The spectrogram pair (csrc/stft.hip) and the layout moves, row-layout reductions and element-wise maps of csrc/dualpath.hip at kernel
level against float64.  The C entry points are called through fqss_amd._lib with explicit pointers and leading dimensions.

Entry points covered: fqss_stft, fqss_istft, fqss_istft_bwd, fqss_transpose2d, fqss_dp_segment_fwd / _bwd, fqss_dp_merge_fwd / _bwd,
fqss_ola2_fwd / _bwd, fqss_permute4, fqss_permute4_ld, fqss_gnrows_fwd / _bwd, fqss_bcast_add, fqss_bcast_sum, fqss_colsum,
fqss_unary_fwd, fqss_unary_rows_fwd, fqss_unary2_fwd, fqss_unary_bwd, fqss_glu_fwd / _bwd, fqss_div_fwd / _bwd, fqss_embedding_fwd / _bwd,
and the deterministic-mode form of the fp32 gradient atomics of k_colsum, k_gnrows_bwd_reduce and k_embedding_bwd.

Measured on the MI355X: largest e_elem / e_norm over the well-conditioned cases of a family (two runs; the sums through fp32 atomics
differ from run to run), beside torch fp32 on the CPU on the same cases, the bound (BOUND below) and its factor over the measurement:
                                         kernel               fp32                 bound                factor
  fqss_stft            z                 8.84e-7 / 1.36e-7    8.05e-7 / 1.29e-7    3.1e-6 / 4.8e-7      3.5 / 3.5   (N = 2048)
  fqss_istft           y                 9.51e-7 / 1.43e-7    9.92e-7 / 1.41e-7    3.3e-6 / 5e-7        3.5 / 3.5   (N = 1024; e_norm N = 32, L = 15)
  fqss_istft_bwd       gz                1.20e-6 / 1.42e-7    8.45e-7 / 1.37e-7    4.2e-6 / 5e-7        3.5 / 3.5   (N = 2048)
    <istft(z), g> - <z, istft_bwd(g)>    1.6e-8 of ||y|| ||g|| + ||gz|| ||z||; bound = the larger e_norm bound of the case (Cauchy-Schwarz), 5e-7
  fqss_gnrows_fwd      y                 6.76e-7 / 9.93e-8    5.87e-7 / 6.17e-8    2.4e-6 / 3.5e-7      3.6 / 3.5
                       rstd              2.31e-7 / 8.45e-8    2.31e-7 / 9.53e-8    8e-7 / 3e-7          3.5 / 3.6
                       mean, per unit of std   <= 2.5e-8 (offset 30: 8.2e-7, 1000: 2.5e-5)      (|mean| / std + 1) 2^-24: one rounding to fp32
  fqss_gnrows_bwd      gx                2.19e-6 / 1.06e-7    1.54e-6 / 7.58e-8    7.6e-6 / 3.7e-7      3.5 / 3.5   (B = 16, C = 8: 48 elements per sample)
                       ggamma            1.62e-6 / 1.16e-6    1.40e-6 / 1.17e-6    5.6e-6 / 4e-6        3.5 / 3.4   (33 100 rows of 2: fp32 serial sums + atomics)
                       gbeta             1.39e-6 / 9.87e-7    3.67e-7 / 1.68e-7    4.8e-6 / 3.4e-6      3.5 / 3.4   (the same case)
  fqss_bcast_sum                         2.39e-7 / 4.22e-8    2.39e-7 / 4.65e-8    8.4e-7 / 1.5e-7      3.5 / 3.6
  fqss_colsum                            7.88e-7 / 1.34e-7    3.03e-7 / 8.15e-8    2.8e-6 / 4.7e-7      3.6 / 3.5   (16 fp32 atomics per column at 1000 rows;
                                                                                                        deterministic mode: 2.0e-7 / 9.4e-8)
  fqss_unary_fwd       tanh              9.30e-8 / 2.37e-8    4.05e-8 / 2.03e-8    3.3e-7 / 8.3e-8      3.5 / 3.5
                       sigmoid           1.36e-7 / 3.79e-8    1.36e-7 / 3.73e-8    4.8e-7 / 1.3e-7      3.5 / 3.4
                       GELU              3.43e-7 / 3.73e-8    3.43e-7 / 3.66e-8    1.2e-6 / 1.3e-7      3.5 / 3.5
  fqss_unary_bwd       tanh'             3.02e-7 / 4.10e-8    3.02e-7 / 4.10e-8    1.05e-6 / 1.4e-7     3.5 / 3.4
                       sigmoid'          3.78e-7 / 4.33e-8    3.78e-7 / 4.33e-8    1.3e-6 / 1.5e-7      3.4 / 3.5
                       GELU'             5.33e-7 / 4.79e-8    4.28e-7 / 4.77e-8    1.9e-6 / 1.7e-7      3.6 / 3.5
  fqss_glu_fwd / _bwd  y                 4.06e-7 / 4.41e-8    4.06e-7 / 4.43e-8    1.4e-6 / 1.5e-7      3.4 / 3.4
                       ga (first half)   4.54e-7 / 4.54e-8    4.54e-7 / 4.55e-8    1.6e-6 / 1.6e-7      3.5 / 3.5
                       gb (second half)  1.76e-6 / 9.76e-8    1.93e-6 / 9.77e-8    6.2e-6 / 3.4e-7      3.5 / 3.5
  fqss_div_bwd         ga, gb            2.58e-7 / 2.50e-8, 4.62e-7 / 4.15e-8 (= fp32)     9e-7 / 8.7e-8, 1.6e-6 / 1.45e-7      3.5
  fqss_embedding_bwd   gw                7.46e-6 / 1.73e-6    4.23e-6 / 9.79e-7    2.6e-5 / 6e-6        3.5 / 3.5   (5000 fp32 atomics on one row; 50 indices:
                                                                                                        <= 5.5e-7; deterministic mode 1.9e-7 / 5.1e-8)
Bit-exact, no bound: fqss_transpose2d, fqss_dp_segment_*, fqss_dp_merge_*, fqss_ola2_*, fqss_permute4(_ld), fqss_bcast_add, fqss_div_fwd,
fqss_embedding_fwd, fqss_unary_fwd kind 2 (x / p) and its backward, fqss_unary2_fwd kinds 4 - 7, fqss_unary_rows_fwd against fqss_unary_fwd.
gnrows offset cases (bound = COND = 4 x torch fp32's own error on the case; measured kernel / fp32 ratio, after the fix below): offset 30:
y 0.28 / 0.27, rstd 1.0 / 2.1, gx 1.8 / 0.9, ggamma 0.16 / 0.12; offset 1000: y 0.13 / 0.24, rstd 1.0 / 0.9, gx 0.10 / 0.09, ggamma 0.04 / 0.17.

Defects found and fixed with this file:
  1. k_gnrows_stats squared and summed in fp32 per lane (q += v * v) before its fp64 wave sum: each square lost |mean|^2 2^-24, which
     E[x^2] - mean^2 turns into an error of the variance.  Measured on the library of the parent commit against the bound 4 x fp32:
     offset 1000, (2,200) K3 S5: rstd 1.96e-3 (bound 2.5e-7), y 1.18e-2 (5.4e-4), gx 8.25e-3 (3.7e-5), ggamma 6.65e-3 (1.5e-3); (2,64) K4 S7:
     rstd 1.55e-4 (1.8e-7), y 5.72e-4 (2.2e-4), gx 6.00e-4 (6.4e-5); offset 30: rstd 9.5e-7 (1.2e-7), gx 4.0e-6 (2.7e-6).  The lanes now
     convert each element to fp64 first; after: rstd 5.6e-8, y 3.3e-5, gx 8.5e-7, ggamma 6.6e-5 on the first case, every ratio <= 2.1.
  2. fqss_istft / fqss_istft_bwd accepted hop = n_fft, where the periodic Hann envelope w^2 is zero at n = 0 and the output could only be
     non-finite: both entries now require 2 hop <= n_fft (FQSS_EINVAL in front of the launch).

Mutation floors: smallest e_elem the wrong kernel gives over the cases where it is not void.  Measured twice: on the MI355X with scratch
copies of the library carrying ONE mutation each (built outside the package, never committed: every copy fails this file, in exactly the
tests that run the mutated line -- 3 for the radix-2 tail, 4 for the radix-4 tail, 12 for each of the other stft.hip mutations, 19 / 2
for n without C / eps, 3 / 3 / 1 / 1 / 1 / 1 for segment, merge, bcast, GLU, round and GELU'), and in float64 on this file's operands on
the CPU, where fft_lds is restated stage by stage in complex128 for the two tail mutations.  The two agree to the digits shown; the CPU
form is asserted 10 x above the bound in every non-void case of every run (floor() / differs() below):
radix-2 tail skipped (N = 16, 128, 1024): z 1.7, y 2.3, gz 1.3; radix-4 tail's second twiddle from pos (N = 32, 256, 2048): z 2.7, y 1.2, gz
2.2; right reflection 2 L - i: z 0.40 with the index clamped (the mutated kernel reads x[L]: the NaN padding, z not finite); factor 2 of c_k
dropped: gz 1.0; frame offset t + 1 in the overlap-add: y 2.4; gnrows sample map of the other layout: y 0.60, gx 0.29 (B > 1; CPU form only:
r / X % B is the same map as (r % RB) / X, the other layout's X is not); n without the factor C: y 1.3 (C > 1); eps omitted (input of scale
1e-4): y 2.5, rstd 1.2; odd trailing Bp element dropped: 1.0; colsum last row dropped: 1.1e-3 (one of 1000 rows of mean 0.3; 400 x the
bound); (1 - s) dropped in the GLU gradient: 1.7; the pdf term of GELU' dropped: 1.2; b for b^2 in the divide gradient: 0.89; a duplicate
index lost: 6.2e-2.  Bit-exact families (a differing element count instead of a floor): (s & 1) P dropped in segment: >= 3 of 8 elements
(void where T <= P: the odd chunks hold padding only); spk and n swapped in merge: >= 16 of 20 (nspk > 1 and N > 1); rintf replaced by
roundf: the 7 ties.
Void by construction: `bin-0 imaginary part not zeroed in k_istft_frames` -- the real part of the inverse transform of the
Hermitian-filled spectrum does not depend on Im X_0 (element 0 is the `a` side of every butterfly of fft_lds, so it only reaches imaginary
parts): test_istft_ignores_bin0_imaginary_part asserts the bit-identical output instead.

Layout under test.  Operands sit in NaN-filled flat buffers between guard floats, row padding [cols, ld) stays NaN (a read of it poisons
the result); outputs are NaN-filled buffers.  After each call: guards, everything outside an output's rows and its padding columns still
NaN (fqss_permute4_ld documents that it writes zeros there: exactly that is asserted), every in-range element finite, every operand
bit-identical to what was uploaded.

References: plain float64 torch on the CPU, built from the formulas in the kernels' header comments (test_references_on_cpu ties them to
float64 torch.stft / torch.istft, F.group_norm, oracle.dptnet_oracle and autograd).  e_elem = max |got - ref| / rms(ref), e_norm =
||got - ref|| / ||ref||; the yardstick is the same operation in torch fp32 on the CPU, printed beside every kernel figure ("MEAS" lines)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle.dptnet_oracle as DO
from tests.test_gpu_kernels import _ref_spec

K = None
_lib = None
DEV = "cuda"
NAN = float("nan")
INF = float("inf")
EINVAL = -22
G = 64                                   # guard floats on either side of every buffer
F64 = torch.float64
C128 = torch.complex128

# ---------------------------------------------------------------------------------------------------------------------------- bounds
# per family and tensor: (e_elem bound, e_norm bound), at most 4 x the largest figure measured on the MI355X over the family's
# well-conditioned cases (see the table above); the gnrows offset cases take COND x the fp32 yardstick's own error on the same case
BOUND = {
    "stft": {"z": (3.1e-6, 4.8e-7)},
    "istft": {"y": (3.3e-6, 5e-7), "gz": (4.2e-6, 5e-7)},
    "gnrows": {"y": (2.4e-6, 3.5e-7), "rstd": (8e-7, 3e-7), "gx": (7.6e-6, 3.7e-7), "ggamma": (5.6e-6, 4e-6), "gbeta": (4.8e-6, 3.4e-6)},
    "bcast": {"sum": (8.4e-7, 1.5e-7)},
    "colsum": {"out": (2.8e-6, 4.7e-7)},
    "unary": {"tanh": (3.3e-7, 8.3e-8), "sigmoid": (4.8e-7, 1.3e-7), "gelu": (1.2e-6, 1.3e-7), "dtanh": (1.05e-6, 1.4e-7),
              "dsigmoid": (1.3e-6, 1.5e-7), "dgelu": (1.9e-6, 1.7e-7)},
    "glu": {"y": (1.4e-6, 1.5e-7), "ga": (1.6e-6, 1.6e-7), "gb": (6.2e-6, 3.4e-7)},
    "div": {"ga": (9e-7, 8.7e-8), "gb": (1.6e-6, 1.45e-7)},
    "emb": {"gw": (2.6e-5, 6e-6)},
}
COND = 4.0                               # offset cases (|mean| / std of 30 and 1000): bound = COND x the fp32 yardstick's error on that case
MEAN_ULP = 2.0 ** -24                    # the statistics' mean is rounded once to fp32: |mean| 2^-24, stated per unit of std


def _gpu_fixture():
    global K, _lib
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from fqss_amd import _lib as lib
    from fqss_amd import kernels
    K, _lib = kernels, lib


@pytest.fixture(scope="module")
def _gpu():
    _gpu_fixture()
    yield


def gpu(fn):
    """a test of this file that needs the device (test_references_on_cpu does not)"""
    return pytest.mark.gpu(pytest.mark.usefixtures("_gpu")(fn))


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def errs(a, ref):
    """(max |a - ref| / rms(ref), ||a - ref|| / ||ref||) of a against a float64 reference; a non-finite a counts as infinitely far"""
    a = a.double().cpu()
    if not bool(torch.isfinite(a).all()):
        return INF, INF
    d = a - ref
    return float(d.abs().max() / rms(ref)), float(d.norm() / ref.norm())


def stream():
    return torch.cuda.current_stream().cuda_stream


def refused(name, *args, who=None):
    """the entry returns FQSS_EINVAL and fqss_last_error names it (who: the helper that speaks for it)"""
    rc = _lib._bind(name)(*args)
    msg = _lib.load().fqss_last_error().decode()
    torch.cuda.synchronize()
    assert rc == EINVAL and (who or name) in msg, (name, rc, msg)
    return msg


def _bits(t):
    return t.view(torch.int64 if t.dtype in (torch.float64, torch.int64) else torch.int32)


def pad4(M, extra=4):
    """a 16-B row stride with at least `extra` padding floats behind M"""
    return (M + 3) // 4 * 4 + extra


class Blk:
    """[R][M] floats with row stride ld, `off` floats into a NaN-filled flat device buffer that begins and ends with G guard floats (the
    buffer is 256-B aligned: the base is 16-B aligned iff off % 4 == 0).  fill: an operand (its buffer is snapshot for unchanged());
    without it an output"""

    def __init__(self, R, M, ld=None, off=0, fill=None):
        ld = M if ld is None else ld
        assert ld >= M
        self.R, self.M, self.ld, self.o = R, M, ld, G + off
        self.buf = torch.full((self.o + R * ld + G,), NAN, device=DEV)
        assert self.buf.data_ptr() % 256 == 0
        self.view = self.buf.as_strided((R, M), (ld, 1), self.o)
        self.padv = self.buf.as_strided((R, ld - M), (ld, 1), self.o + M)
        self.ptr = self.buf.data_ptr() + 4 * self.o
        self.before = None
        if fill is not None:
            self.view.copy_(fill.reshape(R, M))
            self.before = self.buf.clone()

    def unchanged(self):
        return bool(torch.equal(_bits(self.buf), _bits(self.before)))

    def written(self, pad="nan"):
        """[0, M) of every row finite, the guards NaN; the padding columns [M, ld) of all rows but the last still NaN ("nan") or zero
        ("zero": fqss_permute4_ld); behind the last row's M elements nothing may be written ("nan"), or its padding too is zero"""
        end = self.o + (self.R - 1) * self.ld + (self.ld if pad == "zero" else self.M)
        ok = bool(torch.isfinite(self.view).all()) and bool(torch.isnan(self.buf[:self.o]).all()) and bool(torch.isnan(self.buf[end:]).all())
        if self.ld > self.M:
            ok = ok and (bool((self.padv == 0).all()) if pad == "zero" else bool(torch.isnan(self.padv).all()))
        return ok

    def untouched(self):
        return bool(torch.isnan(self.buf).all())

    def cpu(self, *shape):
        return self.view.cpu().reshape(*shape)


class Vec:
    """n elements between G NaN guards; fill: a tensor or a scalar (NaN: an output)"""

    def __init__(self, n, fill=NAN, dtype=torch.float32):
        self.buf = torch.full((n + 2 * G,), NAN, device=DEV, dtype=dtype)
        self.t = self.buf[G:G + n]
        if isinstance(fill, torch.Tensor):
            self.t.copy_(fill.reshape(-1).to(dtype))
        else:
            self.t.fill_(fill)
        self.ptr = self.t.data_ptr()
        self.before = self.buf.clone()

    def guards(self):
        return bool(torch.isnan(self.buf[:G]).all()) and bool(torch.isnan(self.buf[-G:]).all())

    def written(self):
        return self.guards() and bool(torch.isfinite(self.t).all())

    def unchanged(self):
        return bool(torch.equal(_bits(self.buf), _bits(self.before)))

    def untouched(self):
        return bool(torch.isnan(self.buf).all())

    def cpu(self, *shape):
        t = self.t.cpu()
        return t.reshape(*shape) if shape else t


def all_unchanged(**ops):
    for name, o in ops.items():
        assert o.unchanged(), f"operand {name} changed"


def measure(fam, name, got, ref, ref32, tag, fails, cond=None, bound=None):
    """print e_elem / e_norm of `got` beside torch fp32's, collect a missed bound.  cond: an offset case -- the bound is COND x the fp32
    yardstick's own error on this case; bound: an explicit (e_elem, e_norm) pair"""
    e_elem, e_norm = errs(got, ref)
    f_elem, f_norm = errs(ref32, ref) if ref32 is not None else (NAN, NAN)
    if bound is None:
        bound = (COND * f_elem, COND * f_norm) if cond else BOUND[fam][name]
    print(f"MEAS {fam} {name} e_elem {e_elem:.2e} e_norm {e_norm:.2e} fp32 {f_elem:.2e} {f_norm:.2e} bound {bound[0]:.1e} {bound[1]:.1e}"
          f"{' cond' if cond else ''} | {tag}")
    if not (e_elem <= bound[0] and e_norm <= bound[1]):
        fails.append((tag, name, e_elem, e_norm, bound))
    return bound


def floor(fam, name, mut, ref, what, tag, bound=None):
    """the bound stays 10 x below what the wrong kernel `what` gives on this case's operands (computed in float64 on the CPU)"""
    fl = errs(mut, ref)[0]
    b = (bound or BOUND[fam][name])[0]
    print(f"FLOOR {fam} {name} {what} {fl:.2e} (bound {b:.1e}) | {tag}")
    assert b * 10 <= fl, (tag, what, name, fl, b)


def differs(mut, ref, what, tag):
    """a bit-exact check can fail: the wrong kernel `what` moves at least one element of this case"""
    n = int((mut.double() != ref.double()).sum())
    print(f"FLOOR exact {what}: {n} of {ref.numel()} elements differ | {tag}")
    assert n > 0, (tag, what)


def exact(got, ref64, what):
    """bit-exact data movement: got equals the float64 reference rounded once to fp32"""
    assert bool(torch.equal(got.cpu(), ref64.float())), what


# ===================================================================================================================== spectrogram pair
def hann(N, dtype=F64):
    """the periodic Hann window the product uses (torch.hann_window's fp32 values)"""
    return torch.hann_window(N).to(dtype)


def fft_emul(v, inverse=False, mut=None):
    """fft_lds of csrc/stft.hip stage by stage in complex128 (its fused passes apply the same butterflies): bit-reversed store, radix-2
    DIT stages st = 0 .. logn - 1 with twiddle tw[pos * (N >> (st + 1))], no 1 / N.  mut "r2tail": the single radix-2 stage that remains
    when logn % 3 == 1 is skipped; "r4tw": in the radix-4 tail (logn % 3 == 2) the second twiddle of the last stage is taken from pos
    instead of pos + h"""
    N = v.shape[-1]
    logn = N.bit_length() - 1
    rev = torch.tensor([int(format(i, f"0{logn}b")[::-1], 2) for i in range(N)])
    s = v.to(C128)[..., rev]
    ang = -2.0 * math.pi * torch.arange(N // 2, dtype=F64) / N
    tw = torch.complex(torch.cos(ang), torch.sin(ang) * (-1.0 if inverse else 1.0))
    lead = s.shape[:-1]
    for st in range(logn):
        last = st == logn - 1
        if mut == "r2tail" and logn % 3 == 1 and last:
            continue
        h = 1 << st
        pos = torch.arange(h)
        if mut == "r4tw" and logn % 3 == 2 and last:
            pos = pos % (h // 2)
        w = tw[pos * (N >> (st + 1))]
        s = s.reshape(*lead, N // (2 * h), 2, h)
        a, c = s[..., 0, :], s[..., 1, :] * w
        s = torch.stack([a + c, a - c], -2).reshape(*lead, N)
    return s


def reflect_idx(T, N, hop, pad, L, right_2L=False):
    """sample index of element n of frame f of the signal reflect-padded about 0 and L - 1 (right_2L: the wrong map 2 L - i on the right)"""
    i = torch.arange(T)[:, None] * hop + torch.arange(N)[None, :] - pad
    i = torch.where(i < 0, -i, i)
    r = (2 * L - i).clamp(max=L - 1) if right_2L else 2 * (L - 1) - i
    return torch.where(i >= L, r, i)


def _cdtype(dtype):
    return C128 if dtype == F64 else torch.complex64


def stft_ref(x, N, hop, T, pad, dtype=F64, fft=torch.fft.fft, right_2L=False):
    """z[row][0/1][f][k] = (1 / sqrt N) FFT_k(w[n] x2[f hop + n]), k < N/2, x2 = x reflect-padded by `pad` on the left (stft.hip:96)"""
    x = x.to(dtype)
    fr = x[:, reflect_idx(T, N, hop, pad, x.shape[-1], right_2L)] * hann(N, dtype)
    Z = fft(fr.to(_cdtype(dtype)))[..., :N // 2] / math.sqrt(N)
    return torch.stack([Z.real, Z.imag], 1)


def envelope(N, hop, dtype=F64):
    w = hann(N, dtype)
    return (w * w).view(N // hop, hop).sum(0)


def istft_ref(z, N, hop, pad, length, dtype=F64, ifft=torch.fft.ifft, frame_off=2):
    """y[row][j] = sum_t fr[row][t][n - (t + 2) hop] / env[n % hop], n = j + N/2 + pad, fr[t] = w sqrt(N) irfft(Z_t) with a zero Nyquist
    bin and the imaginary part of bin 0 ignored (stft.hip:118, 138).  frame_off: the wrong kernel that places frame t at (t + 1) hop"""
    rows, _, T, H = z.shape
    re, im = z[:, 0].to(dtype), z[:, 1].to(dtype).clone()
    im[..., 0] = 0
    X = torch.zeros(rows, T, N, dtype=_cdtype(dtype))
    X[..., :H] = torch.complex(re, im)
    X[..., H + 1:] = X[..., 1:H].conj().flip(-1)
    fr = ifft(X).real.to(dtype) * math.sqrt(N) * hann(N, dtype)
    total = max((T + 4) * hop + N, length + N + pad)
    buf = torch.zeros(rows, total, dtype=dtype)
    posn = ((torch.arange(T) + frame_off) * hop)[:, None] + torch.arange(N)[None, :]
    buf.index_add_(1, posn.reshape(-1), fr.reshape(rows, -1))
    n = torch.arange(length) + N // 2 + pad
    return buf[:, n] / envelope(N, hop, dtype)[n % hop]


def istft_bwd_ref(g, N, hop, pad, T, dtype=F64, fft=torch.fft.fft, c2=2.0):
    """gz[row][0/1][t][k] = c_k FFT_k(w[m] g[row][(t + 2) hop + m - N/2 - pad] / env), c_0 = 1 / sqrt N (imaginary part 0), c_k = 2 / sqrt N
    (stft.hip:155).  c2: the factor 2 (1: dropped)"""
    g = g.to(dtype)
    rows, length = g.shape
    n = ((torch.arange(T) + 2) * hop)[:, None] + torch.arange(N)[None, :]
    j = n - N // 2 - pad
    ok = (j >= 0) & (j < length)
    v = torch.where(ok, g[:, j.clamp(0, length - 1)] / envelope(N, hop, dtype)[n % hop], torch.zeros((), dtype=dtype)) * hann(N, dtype)
    Gz = fft(v.to(_cdtype(dtype)))[..., :N // 2] / math.sqrt(N)
    c = torch.full((N // 2,), c2, dtype=dtype)
    c[0] = 1.0
    re, im = Gz.real * c, Gz.imag * c
    im[..., 0] = 0
    return torch.stack([re, im], 1)


def spec_shortest_L(N, hop, pad):
    """the shortest signal fqss_stft accepts with T = ceil(L / hop): pad < L and the right reflection (T - 1) hop + N - 1 - pad - (L - 1) < L"""
    L = 2
    while not (pad < L and (-(-L // hop) - 1) * hop + N - 1 - pad - (L - 1) < L):
        L += 1
    return L


def spec_tables(N, hop):
    win, tw, env = K.fft_tables(N, hop, DEV)
    return Vec(N, win), Vec(N, tw), Vec(hop, env)


def spec_case(N, hop, L, rows, ld_extra, seed, fails, tag, floors=True):
    """fqss_stft, fqss_istft and fqss_istft_bwd on one (N, hop, L, rows) with T = ceil(L / hop) frames against the formula references"""
    pad, T, H = hop // 2 * 3, -(-L // hop), N // 2
    wv, tv, ev = spec_tables(N, hop)
    tabs = dict(win=wv, tw=tv, env=ev)
    x, zin, g = rnd(rows, L, seed=seed), rnd(rows, 2, T, H, seed=seed + 1), rnd(rows, L, seed=seed + 2)
    assert float(zin[:, 1, :, 0].abs().min()) > 0          # the bin-0 imaginary plane is non-zero: the kernel must ignore it
    nz = rows * 2 * T * H
    # forward transform
    xb, zb = Blk(rows, L, L + ld_extra, fill=x), Vec(nz)
    _lib.call("fqss_stft", xb.ptr, zb.ptr, wv.ptr, tv.ptr, rows, L, xb.ld, N, hop, T, pad, stream())
    torch.cuda.synchronize()
    assert zb.written(), "z: a NaN inside or a write outside"
    all_unchanged(x=xb, **tabs)
    ref = stft_ref(x, N, hop, T, pad)
    bz = measure("stft", "z", zb.cpu(rows, 2, T, H), ref, stft_ref(x, N, hop, T, pad, torch.float32), tag, fails)
    # inverse and its adjoint
    zi, frb, yb = Vec(nz, zin), Vec(rows * T * N), Blk(rows, L, L + ld_extra)
    _lib.call("fqss_istft", zi.ptr, frb.ptr, yb.ptr, wv.ptr, ev.ptr, tv.ptr, rows, L, yb.ld, N, hop, T, pad, stream())
    torch.cuda.synchronize()
    assert yb.written() and frb.written(), "y / frames: a NaN inside or a write outside"
    all_unchanged(z=zi, **tabs)
    gb, gzb = Blk(rows, L, L + ld_extra, fill=g), Vec(nz)
    _lib.call("fqss_istft_bwd", gb.ptr, gzb.ptr, wv.ptr, ev.ptr, tv.ptr, rows, L, gb.ld, N, hop, T, pad, stream())
    torch.cuda.synchronize()
    assert gzb.written(), "gz: a NaN inside or a write outside"
    all_unchanged(g=gb, **tabs)
    y, gz = yb.cpu(rows, L), gzb.cpu(rows, 2, T, H)
    yref, gzref = istft_ref(zin, N, hop, pad, L), istft_bwd_ref(g, N, hop, pad, T)
    by = measure("istft", "y", y, yref, istft_ref(zin, N, hop, pad, L, torch.float32), tag, fails)
    bg = measure("istft", "gz", gz, gzref, istft_bwd_ref(g, N, hop, pad, T, torch.float32), tag, fails)
    assert bool((gz[:, 1, :, 0] == 0).all()), "gz: the imaginary part of bin 0 must be exactly 0"
    # <istft(z), g> = <z, istft_bwd(g)> in float64 on the kernels' own outputs (z with its bin-0 imaginary part, which gz meets with 0):
    # by Cauchy-Schwarz each side is off by at most e_norm ||y|| ||g|| resp. e_norm ||gz|| ||z||
    lhs, rhs = float((y.double() * g.double()).sum()), float((zin.double() * gz.double()).sum())
    e_dot = abs(lhs - rhs) / (float(yref.norm() * g.double().norm()) + float(gzref.norm() * zin.double().norm()))
    print(f"MEAS istft dot e {e_dot:.2e} bound {max(by[1], bg[1]):.1e} | {tag}")
    if not e_dot <= max(by[1], bg[1]):
        fails.append((tag, "dot-product identity", e_dot))
    if not floors:
        return
    logn = N.bit_length() - 1
    for mut in (["r2tail"] if logn % 3 == 1 else []) + (["r4tw"] if logn % 3 == 2 else []):
        what = {"r2tail": "radix-2 tail skipped", "r4tw": "radix-4 tail: second twiddle from pos"}[mut]
        f = lambda v, m=mut: fft_emul(v, False, m)                       # noqa: E731
        fi = lambda v, m=mut: fft_emul(v, True, m) / N                    # noqa: E731
        floor("stft", "z", stft_ref(x, N, hop, T, pad, fft=f), ref, what, tag, bz)
        floor("istft", "y", istft_ref(zin, N, hop, pad, L, ifft=fi), yref, what, tag, by)
        floor("istft", "gz", istft_bwd_ref(g, N, hop, pad, T, fft=f), gzref, what, tag, bg)
    floor("stft", "z", stft_ref(x, N, hop, T, pad, right_2L=True), ref, "right reflection 2 L - i", tag, bz)
    floor("istft", "gz", istft_bwd_ref(g, N, hop, pad, T, c2=1.0), gzref, "factor 2 of c_k dropped", tag, bg)
    floor("istft", "y", istft_ref(zin, N, hop, pad, L, frame_off=1), yref, "frame offset t + 1", tag, by)


SPEC_N = [8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096]


@gpu
@pytest.mark.parametrize("N", SPEC_N)
def test_spectrogram_pair_against_fp64(N):
    """hop = N / 4, pad = hop // 2 * 3 (the model's framing): the shortest signal fqss_stft accepts (a frame reflects at both ends) and
    L = 2 N + 3 (row stride > L), rows 1 and 3; N = 64 also L = 5 hop.  log2 N mod 3 = 0, 1, 2 over the ten sizes: the radix-8 passes
    alone, the radix-2 tail and the radix-4 tail of fft_lds"""
    hop = N // 4
    pad = hop // 2 * 3
    Ls = [(spec_shortest_L(N, hop, pad), 0), (2 * N + 3, 5)] + ([(5 * hop, 0)] if N == 64 else [])
    fails = []
    for L, ld_extra in Ls:
        for rows in (1, 3):
            spec_case(N, hop, L, rows, ld_extra, 1000 + N + L + rows, fails, f"N {N} hop {hop} L {L} rows {rows} ld +{ld_extra}")
    assert not fails, fails


@gpu
def test_spectrogram_pair_hop_half():
    """hop = N / 2 (envelope sin^4 + cos^4 >= 1/2) for all three entries against the same formula references"""
    fails = []
    spec_case(32, 16, 2 * 32 + 3, 3, 5, 77, fails, "N 32 hop 16 L 67 rows 3 ld +5")
    assert not fails, fails


@gpu
def test_istft_long_signal_grid_stride():
    """length above 1024 * 1024 at N = 8, one row: the grid of k_istft_ola is capped at 1024 workgroups and its grid-stride loop runs on"""
    N, hop, L = 8, 2, 1024 * 1024 + 5
    fails = []
    spec_case(N, hop, L, 1, 0, 5, fails, f"N 8 hop 2 L {L} rows 1", floors=False)
    assert not fails, fails


@gpu
def test_istft_ignores_bin0_imaginary_part():
    """the output of fqss_istft is bit-identical whether the imaginary plane of bin 0 holds noise or zeros.  (The real part of a complex
    inverse transform of a Hermitian-filled spectrum does not depend on Im X_0 -- in fft_lds element 0 is the `a` side of every butterfly,
    so Im X_0 only ever reaches imaginary parts: the mutation `bin-0 imaginary part not zeroed` changes no output bit and has no floor.)"""
    N, hop, L, rows = 64, 16, 131, 2
    pad, T, H = hop // 2 * 3, -(-L // hop), N // 2
    wv, tv, ev = spec_tables(N, hop)
    zin = rnd(rows, 2, T, H, seed=3)
    z0 = zin.clone()
    z0[:, 1, :, 0] = 0
    ys = []
    for z in (zin, z0):
        zi, frb, yb = Vec(z.numel(), z), Vec(rows * T * N), Blk(rows, L, L + 3)
        _lib.call("fqss_istft", zi.ptr, frb.ptr, yb.ptr, wv.ptr, ev.ptr, tv.ptr, rows, L, yb.ld, N, hop, T, pad, stream())
        torch.cuda.synchronize()
        assert yb.written() and zi.unchanged()
        ys.append(yb.cpu(rows, L))
    assert bool(torch.equal(_bits(ys[0]), _bits(ys[1])))


@gpu
def test_spectrogram_pair_refuses_bad_arguments():
    """every FQSS_REQUIRE of the three entries, all in front of the launch: FQSS_EINVAL and nothing written"""
    N, hop, L, rows = 64, 16, 131, 2
    pad, T = hop // 2 * 3, -(-L // hop)
    wv, tv, ev = spec_tables(N, hop)
    xb = Blk(rows, L, L + 3, fill=rnd(rows, L))
    z, fr, yb = Vec(rows * 2 * T * N // 2), Vec(rows * T * N), Blk(rows, L, L + 3)
    zin = Vec(rows * 2 * T * N // 2, rnd(rows * T * N))

    def st(x=xb.ptr, rows=rows, L=L, ld=xb.ld, N=N, hop=hop, T=T, pad=pad, who=None):
        # (the preconditions of fqss_stft restated: no case of this test may pass them and launch)
        assert x is None or not (N in SPEC_N and hop > 0 and N % hop == 0 and 0 < rows <= 65535 and T > 0 and L > 1 and ld >= L
                                 and 0 <= pad < L and (T - 1) * hop + N - 1 - pad - (L - 1) < L)
        return refused("fqss_stft", x, z.ptr, wv.ptr, tv.ptr, rows, L, ld, N, hop, T, pad, stream(), who=who)

    def inv_ok(p, rows, L, ld, N, hop, T, pad):
        return p is not None and N in SPEC_N and hop > 0 and N % hop == 0 and 0 < rows <= 65535 and T > 0 and L > 0 and ld >= L and pad >= 0 and 2 * hop <= N

    def ist(zp=zin.ptr, rows=rows, L=L, ld=yb.ld, N=N, hop=hop, T=T, pad=pad, who=None):
        assert not inv_ok(zp, rows, L, ld, N, hop, T, pad)
        return refused("fqss_istft", zp, fr.ptr, yb.ptr, wv.ptr, ev.ptr, tv.ptr, rows, L, ld, N, hop, T, pad, stream(), who=who)

    def bwd(gp=xb.ptr, rows=rows, L=L, ld=xb.ld, N=N, hop=hop, T=T, pad=pad, who=None):
        assert not inv_ok(gp, rows, L, ld, N, hop, T, pad)
        return refused("fqss_istft_bwd", gp, z.ptr, wv.ptr, ev.ptr, tv.ptr, rows, L, ld, N, hop, T, pad, stream(), who=who)
    for f in (st, ist, bwd):
        f(None)                                                         # null pointer
        for n_fft in (4, 8192, 96):                                      # (check_fft speaks for the three entries)
            assert "n_fft" in f(N=n_fft, hop=n_fft // 4, who="check_fft")
        assert "hop" in f(hop=24, who="check_fft")                      # hop does not divide n_fft
        f(hop=0, who="check_fft")
        f(rows=0)
        f(rows=65536)
        f(ld=L - 1)
        f(T=0)
    st(pad=L)                                                           # pad >= L
    st(pad=-1)
    st(L=1, ld=1)
    st(T=T + 8)                                                         # the right reflection would be longer than the signal
    st(L=20, ld=20, T=2, pad=0, N=64)                                   # ... one frame longer than twice the signal
    ist(pad=-1)
    bwd(pad=-1)
    ist(L=0)
    bwd(L=0)
    # the zero-envelope hop: with the periodic Hann window and hop = N the envelope is w^2, zero at n = 0; the inverse divides by it.
    # Refused by fqss_istft / fqss_istft_bwd (hops up to N / 2 are meant: N / 4 is the model's, N / 2 still has an envelope >= 1/2)
    assert "hop" in ist(hop=N)
    assert "hop" in bwd(hop=N)
    assert z.untouched() and fr.untouched() and yb.untouched() and xb.unchanged() and zin.unchanged()


@gpu
def test_transpose2d_bit_exact():
    for (Bn, R, C) in [(1, 1, 1), (2, 32, 32), (3, 31, 33), (2, 65, 1), (1, 1, 70), (2, 100, 37)]:
        x = rnd(Bn, R, C, seed=R + C)
        xb, yb = Vec(x.numel(), x), Vec(x.numel())
        _lib.call("fqss_transpose2d", xb.ptr, yb.ptr, Bn, R, C, stream())
        torch.cuda.synchronize()
        assert yb.written() and xb.unchanged()
        assert bool(torch.equal(yb.cpu(Bn, C, R), x.transpose(-1, -2))), (Bn, R, C)
    xb, yb = Vec(4, 1.0), Vec(4)
    refused("fqss_transpose2d", xb.ptr, yb.ptr, 65536, 1, 1, stream())
    refused("fqss_transpose2d", xb.ptr, yb.ptr, 1, 0, 1, stream())
    refused("fqss_transpose2d", None, yb.ptr, 1, 1, 1, stream())
    assert yb.untouched()


# ======================================================================================================================== layout moves
def dp_T_list(Kc):
    P = Kc // 2
    return sorted({1, max(P - 1, 1), P, Kc, Kc + 1, 3 * Kc, 3 * Kc + P, 37})


def chunks_ref(T, Kc):
    """(rest, S) from the oracle's split_feature itself"""
    seg, rest = DO.split_feature(torch.zeros(1, 1, T, dtype=F64), Kc)
    return rest, seg.shape[-1]


def segment_formula(f, Kc, S, drop_odd_shift=False):
    """seg[k][b S + s][n] = fpad[b][n][(s >> 1) K + (s & 1) P + k], fpad = P zeros | f | zeros (dualpath.hip:470)"""
    B, N, T = f.shape
    P = Kc // 2
    s, k = torch.arange(S)[None, :], torch.arange(Kc)[:, None]
    j = (s >> 1) * Kc + (0 if drop_odd_shift else (s & 1) * P) + k - P          # [K, S]
    ok = (j >= 0) & (j < T)
    v = torch.where(ok, f[:, :, j.clamp(0, T - 1)], torch.zeros((), dtype=f.dtype))   # [B, N, K, S]
    return v.permute(2, 0, 3, 1).reshape(Kc, B * S, N)


def segment_ref(f, gseg, Kc):
    """the oracle's split_feature in float64 moved to [K][B S][N] by plain permute, and its autograd"""
    fd = f.double().requires_grad_(True)
    seg, _ = DO.split_feature(fd, Kc)                                     # [B, N, K, S]
    B, N, _, S = seg.shape
    rows = seg.permute(2, 0, 3, 1).reshape(Kc, B * S, N)
    rows.backward(gseg.double())
    return rows.detach(), fd.grad


@gpu
@pytest.mark.parametrize("Kc", [2, 4, 10])
def test_dp_segment_bit_exact(Kc):
    """fqss_dp_segment_fwd / _bwd over T with T % K = 0, T % K = P (rest = K in dp_chunks) and T < P, B in {1, 3}, N in {1, 5}, ld_f > T"""
    P = Kc // 2
    for T in dp_T_list(Kc):
        rest, S = chunks_ref(T, Kc)
        assert K.dp_chunks(T, Kc) == (rest, S), (T, Kc)
        for B in (1, 3):
            for N in (1, 5):
                tag = f"K {Kc} T {T} B {B} N {N} S {S}"
                f, gseg = rnd(B, N, T, seed=T + B + N), rnd(Kc, B * S, N, seed=T + B + N + 1)
                want, gwant = segment_ref(f, gseg, Kc)
                fb, sb = Blk(B * N, T, T + 3, fill=f), Vec(Kc * B * S * N)
                _lib.call("fqss_dp_segment_fwd", fb.ptr, sb.ptr, B, N, T, fb.ld, Kc, S, stream())
                gsb, gfb = Vec(gseg.numel(), gseg), Blk(B * N, T, T + 3)
                _lib.call("fqss_dp_segment_bwd", gsb.ptr, gfb.ptr, B, N, T, gfb.ld, Kc, S, stream())
                torch.cuda.synchronize()
                assert sb.written() and gfb.written(), tag
                all_unchanged(f=fb, gseg=gsb)
                exact(sb.cpu(Kc, B * S, N), want, tag)
                exact(gfb.cpu(B, N, T), gwant, tag + " backward")
                if S > 1 and T > P:       # (void where the odd chunks hold padding only)
                    differs(segment_formula(f.double(), Kc, S, drop_odd_shift=True), want, "(s & 1) P dropped", tag)
    fb, sb = Blk(2, 7, 8, fill=rnd(2, 7)), Vec(4 * 6 * 2)
    bad = [dict(B=0), dict(N=0), dict(T=0), dict(ld=6), dict(Kc=3), dict(Kc=0), dict(S=5), dict(S=0)]
    for kw in bad:
        a = dict(B=1, N=2, T=7, ld=8, Kc=4, S=6)
        a.update(kw)
        for name in ("fqss_dp_segment_fwd", "fqss_dp_segment_bwd"):
            refused(name, fb.ptr, sb.ptr, a["B"], a["N"], a["T"], a["ld"], a["Kc"], a["S"], stream())
    refused("fqss_dp_segment_fwd", fb.ptr, sb.ptr, 1, 2, 7, 8, 4, 4, stream())          # S chunks do not cover the signal
    refused("fqss_dp_segment_fwd", None, sb.ptr, 1, 2, 7, 8, 4, 6, stream())
    assert sb.untouched() and fb.unchanged()


def merge_formula(o, B, nspk, N, Kc, S, swap=False):
    """a[t] = o[s = 2 ((t + P) / K)][k = (t + P) % K], b[t] = o[s = 2 (t / K) + 1][k = t % K] from o [S][B K + k][spk N + n] into
    [B nspk][N][Lm], Lm = (S / 2) K - P (dualpath.hip:511).  swap: the wrong kernel that reads column n nspk + spk"""
    P = Kc // 2
    Lm = (S // 2) * Kc - P
    o5 = o.reshape(S, B, Kc, N, nspk).permute(0, 1, 2, 4, 3) if swap else o.reshape(S, B, Kc, nspk, N)
    t = torch.arange(Lm)
    a = o5[2 * ((t + P) // Kc), :, (t + P) % Kc]                          # [Lm, B, nspk, N]
    b = o5[2 * (t // Kc) + 1, :, t % Kc]
    return tuple(v.permute(1, 2, 3, 0).reshape(B * nspk, N, Lm) for v in (a, b))


def merge_operand(S, B, Kc, nspk, N, seed):
    """o with every (speaker, channel) plane on a level of its own: a swapped spk N + n cannot pass"""
    return rnd(S, B * Kc, nspk * N, seed=seed) + 10.0 * torch.arange(nspk * N)


@gpu
@pytest.mark.parametrize("Kc", [2, 4, 10])
def test_dp_merge_bit_exact(Kc):
    """fqss_dp_merge_fwd / _bwd for nspk 1, 2 and 3 on the (K, S) pairs of the segment test, B in {1, 2}, N in {1, 5}, ld_ab > Lm; ga or
    gb absent through K.dp_merge_bwd"""
    for S in sorted({chunks_ref(T, Kc)[1] for T in dp_T_list(Kc)}):
        Lm = (S // 2) * Kc - Kc // 2
        for nspk in (1, 2, 3):
            for B in (1, 2):
                for N in (1, 5):
                    tag = f"K {Kc} S {S} nspk {nspk} B {B} N {N}"
                    o = merge_operand(S, B, Kc, nspk, N, seed=S + nspk + B + N)
                    od = o.double().requires_grad_(True)
                    aw, bw = merge_formula(od, B, nspk, N, Kc, S)
                    ga, gb = rnd(B * nspk, N, Lm, seed=1), rnd(B * nspk, N, Lm, seed=2)
                    gow, = torch.autograd.grad([aw, bw], od, [ga.double(), gb.double()])
                    ob, ab, bb = Vec(o.numel(), o), Blk(B * nspk * N, Lm, Lm + 3), Blk(B * nspk * N, Lm, Lm + 3)
                    _lib.call("fqss_dp_merge_fwd", ob.ptr, ab.ptr, bb.ptr, B, nspk, N, Kc, S, Lm, ab.ld, stream())
                    gab, gbb, gob = Blk(B * nspk * N, Lm, Lm + 3, fill=ga), Blk(B * nspk * N, Lm, Lm + 5, fill=gb), Vec(o.numel())
                    _lib.call("fqss_dp_merge_bwd", gab.ptr, gbb.ptr, gob.ptr, B, nspk, N, Kc, S, Lm, gab.ld, gbb.ld, stream())
                    torch.cuda.synchronize()
                    assert ab.written() and bb.written() and gob.written(), tag
                    all_unchanged(o=ob, ga=gab, gb=gbb)
                    exact(ab.cpu(B * nspk, N, Lm), aw.detach(), tag + " a")
                    exact(bb.cpu(B * nspk, N, Lm), bw.detach(), tag + " b")
                    exact(gob.cpu(S, B * Kc, nspk * N), gow, tag + " go")
                    if nspk > 1 and N > 1:
                        differs(merge_formula(o.double(), B, nspk, N, Kc, S, swap=True)[0], aw.detach(), "spk and n swapped", tag)
        # one gradient absent (the wrapper supplies zeros)
        o = merge_operand(S, 2, Kc, 2, 5, seed=9)
        od = o.double().requires_grad_(True)
        aw, bw = merge_formula(od, 2, 2, 5, Kc, S)
        ga = rnd(4, 5, Lm, seed=3)
        for which, out in (("ga", aw), ("gb", bw)):
            gow, = torch.autograd.grad(out, od, ga.double(), retain_graph=True)
            go = K.dp_merge_bwd(ga.cuda() if which == "ga" else None, ga.cuda() if which == "gb" else None, 2, 2, 5, Kc, S)
            exact(go, gow, f"K {Kc} S {S} only {which}")
    ob, ab = Vec(4 * 4 * 2, 1.0), Blk(2, 6, 8)
    for kw in (dict(B=0), dict(nspk=0), dict(N=0), dict(Kc=3), dict(S=3), dict(Lm=5), dict(ld=5)):
        a = dict(B=1, nspk=1, N=2, Kc=4, S=4, Lm=6, ld=8)
        a.update(kw)
        refused("fqss_dp_merge_fwd", ob.ptr, ab.ptr, ab.ptr, a["B"], a["nspk"], a["N"], a["Kc"], a["S"], a["Lm"], a["ld"], stream())
        refused("fqss_dp_merge_bwd", ab.ptr, ab.ptr, ob.ptr, a["B"], a["nspk"], a["N"], a["Kc"], a["S"], a["Lm"], a["ld"], a["ld"], stream())
    refused("fqss_dp_merge_fwd", None, ab.ptr, ab.ptr, 1, 1, 2, 4, 4, 6, 8, stream())
    refused("fqss_dp_merge_bwd", None, ab.ptr, ob.ptr, 1, 1, 2, 4, 4, 6, 8, 8, stream())
    assert ab.untouched() and ob.unchanged()


@gpu
def test_ola2_bit_exact():
    """fqss_ola2_fwd / _bwd: out[n][t] = y[n][0][t] + y[n][1][t - 1]; N = 0 is a no-op"""
    for N in (1, 3):
        for L in (1, 2, 257):
            y, g = rnd(N, 2, L, seed=L + N), rnd(N, L + 1, seed=L + N + 1)
            yd = y.double()
            want = F.pad(yd[:, 0], (0, 1)) + F.pad(yd[:, 1], (1, 0))
            gwant = torch.stack([g[:, :L], g[:, 1:]], 1).double()
            yb, ob = Blk(2 * N, L, L + 3, fill=y), Vec(N * (L + 1))
            _lib.call("fqss_ola2_fwd", yb.ptr, ob.ptr, N, L, yb.ld, stream())
            gb, gyb = Vec(g.numel(), g), Blk(2 * N, L, L + 3)
            _lib.call("fqss_ola2_bwd", gb.ptr, gyb.ptr, N, L, gyb.ld, stream())
            torch.cuda.synchronize()
            assert ob.written() and gyb.written(), (N, L)
            all_unchanged(y=yb, g=gb)
            exact(ob.cpu(N, L + 1), want, (N, L))
            exact(gyb.cpu(N, 2, L), gwant, (N, L, "backward"))
    yb, ob, gyb = Blk(2, 4, 5, fill=rnd(2, 4)), Vec(5), Blk(2, 4, 5)
    _lib.call("fqss_ola2_fwd", yb.ptr, ob.ptr, 0, 4, 5, stream())
    _lib.call("fqss_ola2_bwd", ob.ptr, gyb.ptr, 0, 4, 5, stream())
    for a in ((-1, 4, 5), (1, 0, 5), (1, 4, 3)):
        refused("fqss_ola2_fwd", yb.ptr, ob.ptr, *a, stream())
        refused("fqss_ola2_bwd", yb.ptr, gyb.ptr, *a, stream())
    refused("fqss_ola2_fwd", None, ob.ptr, 1, 4, 5, stream())
    refused("fqss_ola2_bwd", None, gyb.ptr, 1, 4, 5, stream())
    torch.cuda.synchronize()
    assert ob.untouched() and gyb.untouched() and yb.unchanged()


PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


@gpu
@pytest.mark.parametrize("C", [1, 3, 4, 5, 64])
def test_permute4_bit_exact(C):
    """fqss_permute4 / fqss_permute4_ld: the six orders of the leading dims of a (3, 4, 5, C) tensor, from a dense source and from a view
    of a row-padded buffer (odd row stride, base one float past a 16-B boundary: for C = 5 the packed 16-B loads of the _ld form run
    unaligned); _ld writes zeros into [C, ld_y) and nothing behind ld_y"""
    D = (3, 4, 5)
    x = rnd(*D, C, seed=C)
    for ld_src, off in ((C, 0), (C + 3 if C % 2 == 0 else C + 2, 1)):
        assert ld_src == C or ld_src % 2 == 1
        xb = Blk(60, C, ld_src, off, fill=x)
        rs = (20 * ld_src, 5 * ld_src, ld_src)
        for p in PERMS:
            dims, st = [D[i] for i in p], [rs[i] for i in p]
            want = x.permute(*p, 3).contiguous()
            yb = Vec(x.numel())
            _lib.call("fqss_permute4", xb.ptr, yb.ptr, *dims, C, *st, stream())
            ld_y = pad4(C, 0) + (4 if p[0] else 0)
            zb = Blk(60, C, ld_y)
            _lib.call("fqss_permute4_ld", xb.ptr, zb.ptr, *dims, C, *st, ld_y, stream())
            torch.cuda.synchronize()
            assert yb.written() and xb.unchanged(), (C, p)
            assert zb.written(pad="zero"), (C, p, "rows finite, zeros in [C, ld_y), nothing behind")
            assert bool(torch.equal(yb.cpu(*dims, C), want)) and bool(torch.equal(zb.cpu(*dims, C), want)), (C, p, ld_src)
    # through the wrapper: the source a non-dense view of a row-padded buffer read in place (dense=False), dense and row-padded output
    big = torch.full((3, 4, 5, C + 3), NAN, device=DEV)
    big[..., :C] = x.to(DEV)
    v = big[..., :C]
    for pad_out in (False, True):
        y = K.permute4(v, (5, 3, 4), (v.stride(2), v.stride(0), v.stride(1)), C, dense=False, pad_out=pad_out)
        assert bool(torch.equal(y.cpu(), x.permute(2, 0, 1, 3))), (C, pad_out)
    xb, zb, z1 = Blk(60, C, fill=x), Blk(60, C, pad4(C)), Blk(60, C, pad4(C), 1)
    a = (3, 4, 5, C, 20 * C, 5 * C, C)
    refused("fqss_permute4_ld", xb.ptr, zb.ptr, *a, pad4(C) - 1, stream())                # ld_y % 4 != 0
    refused("fqss_permute4_ld", xb.ptr, zb.ptr, *a, (C - 1) // 4 * 4, stream())          # ld_y < C
    refused("fqss_permute4_ld", xb.ptr, z1.ptr, *a, pad4(C), stream())                   # y off 16-B alignment
    refused("fqss_permute4_ld", xb.ptr, zb.ptr, 3, 4, 5, 0, 20, 5, 1, 4, stream())
    refused("fqss_permute4", xb.ptr, zb.ptr, 3, 4, 5, 0, 20, 5, 1, stream())
    refused("fqss_permute4", None, zb.ptr, *a, stream())
    _lib.call("fqss_permute4", xb.ptr, zb.ptr, 0, 4, 5, C, 20 * C, 5 * C, C, stream())        # an empty tensor: nothing to do
    _lib.call("fqss_permute4_ld", xb.ptr, zb.ptr, 0, 4, 5, C, 20 * C, 5 * C, C, pad4(C), stream())
    torch.cuda.synchronize()
    assert zb.untouched() and z1.untouched()


# ================================================================================================================= row-layout reductions
GR_EPS = 1e-8                            # the gLN of the Sepformer blocks


def gr_map(R, RB, X):
    """sample of row r (dualpath.hip:588): intra-chunk rows [K][B S][C]: RB = B S, X = S; inter-chunk rows [S][B K][C]: RB = B K, X = K"""
    return (torch.arange(R) % RB) // X


def gr_ref(x, gy, gamma, beta, eps, bmap, B, no_eps=False, n_without_C=False):
    """GroupNorm(1, C) over all rows of a sample of the row matrix x [R][C] and its backward, closed form in float64"""
    R, C = x.shape
    x, gy, gamma, beta = x.double(), gy.double(), gamma.double(), beta.double()
    oh = F.one_hot(bmap, B).double()                                      # [R, B]
    n = oh.sum(0) * (1 if n_without_C else C)
    mean = oh.T @ x.sum(1) / n
    var = (oh.T @ (x * x).sum(1) / n - mean * mean).clamp_(min=0.0)
    rstd = 1.0 / torch.sqrt(var + (0.0 if no_eps else eps))
    xh = (x - mean[bmap, None]) * rstd[bmap, None]
    gh = gy * gamma
    a, b = oh.T @ gh.sum(1) / n, oh.T @ (gh * xh).sum(1) / n
    return {"mean": mean, "rstd": rstd, "y": xh * gamma + beta, "gx": rstd[bmap, None] * (gh - a[bmap, None] - xh * b[bmap, None]),
            "ggamma": (gy * xh).sum(0), "gbeta": gy.sum(0)}


def gr_torch(x, gy, gamma, beta, eps, bmap, B, dtype):
    """the same through F.group_norm on the channel-first tensor [B, C, rows of the sample] and autograd in `dtype`"""
    R, C = x.shape
    idx = torch.stack([torch.nonzero(bmap == b).squeeze(1) for b in range(B)])          # [B, rows per sample]
    X = x.to(dtype)[idx].permute(0, 2, 1).clone().requires_grad_(True)
    ga, be = (t.to(dtype).clone().requires_grad_(True) for t in (gamma, beta))
    y = F.group_norm(X, 1, ga, be, eps)
    y.backward(gy.to(dtype)[idx].permute(0, 2, 1))

    def back(t):
        out = torch.empty(R, C, dtype=dtype)
        out[idx.reshape(-1)] = t.permute(0, 2, 1).reshape(-1, C)
        return out
    xd = X.detach().reshape(B, -1)
    return {"y": back(y.detach()), "gx": back(X.grad), "ggamma": ga.grad, "gbeta": be.grad, "mean": xd.mean(1),
            "rstd": 1.0 / torch.sqrt(xd.var(1, unbiased=False) + eps)}


def gr_operands(R, C, bmap, B, seed, offset=0.3, scale=1.0, const=None):
    """x = scale_b (randn + offset) with a scale (and so a mean) of its own per sample: |mean| / std = offset; gy ~ N(0, 1)"""
    sc = (scale * (0.5 + 0.25 * torch.arange(B)) * (1 - 2 * (torch.arange(B) % 2)))[bmap, None]
    x = torch.full((R, C), const) if const is not None else (rnd(R, C, seed=seed) + offset) * sc
    return x, rnd(R, C, seed=seed + 1), 1.3 * (1 + 0.1 * rnd(C, seed=seed + 2)), 0.2 + 0.1 * rnd(C, seed=seed + 3)


def gr_run(ops, RB, X, B, start, slots=None, eps=GR_EPS):
    """fqss_gnrows_fwd and _bwd with row strides ld > C on x, y, gy and gx; ggamma / gbeta start at `start` (they are added to)"""
    x, gy, gamma, beta = ops
    R, C = x.shape
    xb, gyb, yb, gxb = Blk(R, C, C + 3, fill=x), Blk(R, C, C + 1, fill=gy), Blk(R, C, C + 2), Blk(R, C, C + 5)
    gab, beb, mr, ws = Vec(C, gamma), Vec(C, beta), Vec(2 * B), Vec(2 * B, dtype=F64)
    _lib.call("fqss_gnrows_fwd", xb.ptr, gab.ptr, beb.ptr, yb.ptr, mr.ptr, ws.ptr, R, C, xb.ld, yb.ld, RB, X, B, eps, stream())
    torch.cuda.synchronize()
    assert yb.written() and mr.written() and ws.written() and gxb.untouched()
    all_unchanged(x=xb, gamma=gab, beta=beb)
    out = {"y": yb.cpu(R, C), "mean": mr.cpu(B, 2)[:, 0], "rstd": mr.cpu(B, 2)[:, 1]}
    if slots is None:
        gg, gb = Vec(C, start[0]), Vec(C, start[1])
        pg, pb = gg.ptr, gb.ptr
    else:
        pg, pb = slots[0].data_ptr(), slots[1].data_ptr()
    ws2, mr_before = Vec(2 * B, dtype=F64), mr.buf.clone()
    _lib.call("fqss_gnrows_bwd", gyb.ptr, xb.ptr, gab.ptr, mr.ptr, gxb.ptr, pg, pb, ws2.ptr, R, C, gyb.ld, xb.ld, gxb.ld, RB, X, B, stream())
    torch.cuda.synchronize()
    assert gxb.written() and ws2.written() and bool(torch.equal(_bits(mr.buf), _bits(mr_before)))
    all_unchanged(x=xb, gy=gyb, gamma=gab)
    out["gx"] = gxb.cpu(R, C)
    if slots is None:
        assert gg.written() and gb.written()
        out.update(ggamma=gg.cpu().double() - start[0].double(), gbeta=gb.cpu().double() - start[1].double())
    return out


# id -> B, C, K, S, layout, operand options.  K != S everywhere: the sample map of the other layout is a different map
GR_CASES = {
    "intra (1,1) K2 S3": (1, 1, 2, 3, "intra", {}),
    "inter (1,8) K2 S3": (1, 8, 2, 3, "inter", {}),
    "intra (2,8) K3 S5": (2, 8, 3, 5, "intra", {}),
    "inter (2,8) K3 S5": (2, 8, 3, 5, "inter", {}),
    "intra (2,64) K4 S7": (2, 64, 4, 7, "intra", {}),
    "inter (2,64) K4 S7": (2, 64, 4, 7, "inter", {}),
    "intra (2,200) K3 S5": (2, 200, 3, 5, "intra", {}),
    "inter (2,200) K3 S5": (2, 200, 3, 5, "inter", {}),
    "intra (16,8) K2 S3": (16, 8, 2, 3, "intra", {}),
    "inter (16,1024) K2 S3": (16, 1024, 2, 3, "inter", {}),
    "intra (1,1024) K3 S2": (1, 1024, 3, 2, "intra", {}),
    "intra (2,2) K50 S331: 33 100 rows": (2, 2, 50, 331, "intra", {}),
    "inter (2,2) K331 S50: 33 100 rows": (2, 2, 331, 50, "inter", {}),
    "intra (2,8) K3 S5 tiny input: eps matters": (2, 8, 3, 5, "intra", {"scale": 1e-4}),
    "intra (2,64) K4 S7 mean / std 30": (2, 64, 4, 7, "intra", {"offset": 30.0}),
    "inter (2,200) K3 S5 mean / std 30": (2, 200, 3, 5, "inter", {"offset": 30.0}),
    "intra (2,64) K4 S7 mean / std 1000": (2, 64, 4, 7, "intra", {"offset": 1000.0}),
    "inter (2,200) K3 S5 mean / std 1000": (2, 200, 3, 5, "inter", {"offset": 1000.0}),
}


def gr_geometry(B, Kc, S, layout):
    """(R, RB, X) of the layout and of the other one"""
    R = Kc * B * S
    intra, inter = (R, B * S, S), (R, B * Kc, Kc)
    return (intra, inter) if layout == "intra" else (inter, intra)


def gr_start(C, ref):
    return rnd(C, seed=41, scale=max(rms(ref["ggamma"]), 1e-3)), rnd(C, seed=42, scale=max(rms(ref["gbeta"]), 1e-3))


@gpu
@pytest.mark.parametrize("case", list(GR_CASES))
def test_gnrows_against_fp64(case):
    """fqss_gnrows_fwd / _bwd in both row layouts: y, mean_rstd, gx and the sums ADDED into ggamma / gbeta (non-zero on entry) against
    float64.  The offset cases bound y and the gradients by COND x torch fp32's own error on the case."""
    B, C, Kc, S, layout, opt = GR_CASES[case]
    (R, RB, X), (_, RBo, Xo) = gr_geometry(B, Kc, S, layout)
    assert (R > 32768) == ("33 100" in case)
    bmap = gr_map(R, RB, X)
    ops = gr_operands(R, C, bmap, B, seed=300 + C + B, **opt)
    cond = opt.get("offset", 0.3) > 1.0
    ref, ref32 = gr_ref(*ops, GR_EPS, bmap, B), gr_torch(*ops, GR_EPS, bmap, B, torch.float32)
    start = gr_start(C, ref)
    got = gr_run(ops, RB, X, B, start)
    fails, bounds = [], {}
    mean_err = float(((got["mean"].double() - ref["mean"]) * ref["rstd"]).abs().max())
    mean_bound = (float((ref["mean"].abs() * ref["rstd"]).max()) + 1.0) * MEAN_ULP
    print(f"MEAS gnrows mean |d mean| / std {mean_err:.2e} bound {mean_bound:.2e} | {case}")
    if not mean_err <= mean_bound:
        fails.append((case, "mean", mean_err, mean_bound))
    for n in ("rstd", "y", "gx", "ggamma", "gbeta"):
        if n == "ggamma" and R * C == B:
            continue
        bounds[n] = measure("gnrows", n, got[n], ref[n], ref32[n], case, fails, cond=cond and n != "gbeta")
    assert not fails, fails
    # the wrong kernels
    if B > 1:
        mut = gr_ref(*ops, GR_EPS, gr_map(R, RBo, Xo), B)
        floor("gnrows", "y", mut["y"], ref["y"], "sample map of the other layout", case, bounds["y"])
        floor("gnrows", "gx", mut["gx"], ref["gx"], "sample map of the other layout", case, bounds["gx"])
    if C > 1:
        mut = gr_ref(*ops, GR_EPS, bmap, B, n_without_C=True)
        floor("gnrows", "y", mut["y"], ref["y"], "n without the factor C", case, bounds["y"])
    if "tiny" in case:
        mut = gr_ref(*ops, GR_EPS, bmap, B, no_eps=True)
        floor("gnrows", "y", mut["y"], ref["y"], "eps omitted", case, bounds["y"])
        floor("gnrows", "rstd", mut["rstd"], ref["rstd"], "eps omitted", case, bounds["rstd"])


@gpu
def test_gnrows_constant_input():
    """a constant input: the fp64 sums are exact, var = 0, rstd = 1 / sqrt(eps) and y = beta; every output finite"""
    B, C, Kc, S = 2, 8, 3, 5
    (R, RB, X), _ = gr_geometry(B, Kc, S, "intra")
    bmap = gr_map(R, RB, X)
    ops = gr_operands(R, C, bmap, B, seed=7, const=0.7)
    ref = gr_ref(*ops, GR_EPS, bmap, B)
    start = gr_start(C, ref)
    got = gr_run(ops, RB, X, B, start)
    for n, t in got.items():
        assert bool(torch.isfinite(t).all()), n
    assert bool((got["mean"] == float(np.float32(0.7))).all())
    assert bool((got["rstd"] == 1.0 / np.sqrt(np.float32(GR_EPS))).all()) or float((got["rstd"].double() * math.sqrt(GR_EPS) - 1).abs().max()) <= 2e-7
    assert bool(torch.equal(got["y"], ops[3][None, :].expand(R, C))), "y = beta"
    assert errs(got["gbeta"], ref["gbeta"])[0] <= BOUND["gnrows"]["gbeta"][0]


@gpu
def test_gnrows_refuses_bad_arguments():
    B, C, Kc, S = 2, 8, 3, 5
    R, RB, X = Kc * B * S, B * S, S
    xb, yb = Blk(R, C, C + 3, fill=rnd(R, C)), Blk(R, C, C + 3)
    ga, mr, ws = Vec(C, 1.0), Vec(2 * 17, 0.5), Vec(2 * 17, dtype=F64)

    def fwd(x=xb.ptr, R=R, C=C, ld=C + 3, RB=RB, X=X, B=B):
        refused("fqss_gnrows_fwd", x, ga.ptr, ga.ptr, yb.ptr, mr.ptr, ws.ptr, R, C, ld, ld, RB, X, B, GR_EPS, stream())

    def bwd(x=xb.ptr, R=R, C=C, ld=C + 3, RB=RB, X=X, B=B):
        refused("fqss_gnrows_bwd", x, xb.ptr, ga.ptr, mr.ptr, yb.ptr, ga.ptr, ga.ptr, ws.ptr, R, C, ld, ld, ld, RB, X, B, stream())
    for f in (fwd, bwd):
        f(None)
        f(B=17, RB=17 * S, R=Kc * 17 * S)
        f(RB=RB + 1)                                                     # RB != B X
        f(R=R + 1)                                                       # R % RB != 0
        f(ld=C - 1)
        f(R=0)
    bwd(C=1025, ld=1028)
    assert yb.untouched() and ws.untouched() and xb.unchanged() and ga.unchanged() and mr.unchanged()


@gpu
def test_bcast_add_and_sum():
    """fqss_bcast_add (bit-exact: one fp32 addition) and fqss_bcast_sum (against float64; an odd Bp exercises the trailing element);
    Bp = 0: the sum writes zeros, the add has nothing to do"""
    fails = []
    for (L, Bp, C) in [(1, 1, 1), (7, 2, 5), (33, 5, 64), (4, 1, 3)]:
        tag = f"(L, Bp, C) = ({L}, {Bp}, {C})"
        x, p, g = rnd(L, Bp, C, seed=L), rnd(L, C, seed=L + 1), rnd(L, Bp, C, seed=L + 2)
        xb, pb, zb = Vec(x.numel(), x), Vec(p.numel(), p), Vec(x.numel())
        _lib.call("fqss_bcast_add", xb.ptr, pb.ptr, zb.ptr, L, Bp, C, stream())
        gb, ob = Vec(g.numel(), g), Vec(L * C)
        _lib.call("fqss_bcast_sum", gb.ptr, ob.ptr, L, Bp, C, stream())
        torch.cuda.synchronize()
        assert zb.written() and ob.written()
        all_unchanged(x=xb, p=pb, g=gb)
        exact(zb.cpu(L, Bp, C), x.double() + p.double()[:, None, :], tag)
        ref = g.double().sum(1)
        b = measure("bcast", "sum", ob.cpu(L, C), ref, g.sum(1), tag, fails)
        if Bp % 2 == 1:
            floor("bcast", "sum", g.double()[:, :Bp - 1].sum(1), ref, "odd trailing Bp element dropped", tag, b)
    ob, zb, gb = Vec(3 * 5, 7.0), Vec(8), Vec(8, 1.0)
    _lib.call("fqss_bcast_sum", gb.ptr, ob.ptr, 3, 0, 5, stream())
    _lib.call("fqss_bcast_add", gb.ptr, gb.ptr, zb.ptr, 3, 0, 5, stream())
    torch.cuda.synchronize()
    assert ob.guards() and bool((ob.t == 0).all()) and zb.untouched()
    for name in ("fqss_bcast_add", "fqss_bcast_sum"):
        tail = (gb.ptr,) if name == "fqss_bcast_add" else ()
        refused(name, gb.ptr, *tail, zb.ptr, 2, 2, 0, stream())
        refused(name, gb.ptr, *tail, zb.ptr, -1, 2, 2, stream())
        refused(name, None, *tail, zb.ptr, 2, 2, 2, stream())
    assert zb.untouched()
    assert not fails, fails


@gpu
@pytest.mark.parametrize("C", [1, 2, 8, 9, 64, 200, 256, 257, 1024])
def test_colsum_against_fp64(C):
    """fqss_colsum: out[c] += sum_r g[r][c] with ld > C and a non-zero out, over the column widths CW = 8 .. 256 and more than one column
    block, R below, at and above the 64 rows of a workgroup's slab"""
    fails = []
    for R in (1, 63, 64, 65, 1000):
        tag = f"C {C} R {R}"
        g = rnd(R, C, seed=R + C) + 0.3      # (|mean| / std = 0.3: a column sum that cancels to nothing would make its own rms the yardstick)
        ref = g.double().sum(0)
        start = rnd(C, seed=5, scale=max(rms(ref), 1e-3))
        gb, ob = Blk(R, C, C + 3, fill=g), Vec(C, start)
        _lib.call("fqss_colsum", gb.ptr, ob.ptr, R, C, gb.ld, stream())
        torch.cuda.synchronize()
        assert ob.written() and gb.unchanged()
        b = measure("colsum", "out", ob.cpu().double() - start.double(), ref, g.sum(0), tag, fails)
        if R > 1:
            floor("colsum", "out", g.double()[:-1].sum(0), ref, "last row dropped", tag, b)
    ob = Vec(C, 1.0)
    _lib.call("fqss_colsum", gb.ptr, ob.ptr, 0, C, gb.ld, stream())           # no rows: nothing to add
    refused("fqss_colsum", gb.ptr, ob.ptr, 4, C, C - 1, stream())
    refused("fqss_colsum", gb.ptr, ob.ptr, 4, 0, 4, stream())
    refused("fqss_colsum", None, ob.ptr, 4, C, C, stream())
    torch.cuda.synchronize()
    assert ob.unchanged()
    assert not fails, fails


# ===================================================================================================================== element-wise maps
SPECIAL = [0.0, -0.0, 1e-30, -1e-30, 0.5, -0.5, 5.0, -5.0, 20.0, -20.0, 100.0, -100.0]
SQRT1_2 = 1.0 / math.sqrt(2.0)
UN_P = math.sqrt(24.0)                    # kind 2: q / sqrt(head_dim)


def unary_ref(x, kind, dtype=F64):
    x = x.to(dtype)
    if kind == 0:
        return torch.tanh(x)
    if kind == 1:
        return torch.sigmoid(x)
    if kind == 2:
        return x / torch.tensor(float(np.float32(UN_P)), dtype=dtype)
    return 0.5 * x * (1.0 + torch.erf(x * SQRT1_2))


def unary_bwd_ref(g, y, kind, dtype=F64, no_pdf=False):
    """ATen's tanh_backward / sigmoid_backward on the OUTPUT y; kind 3: y holds the input x, d/dx = Phi(x) + x phi(x)"""
    g, y = g.to(dtype), y.to(dtype)
    if kind == 0:
        return g * (1.0 - y * y)
    if kind == 1:
        return g * (1.0 - y) * y
    if kind == 2:
        return g / torch.tensor(float(np.float32(UN_P)), dtype=dtype)
    cdf = 0.5 * (1.0 + torch.erf(y * SQRT1_2))
    pdf = torch.exp(-0.5 * y * y) / math.sqrt(2.0 * math.pi)
    return g * (cdf + (0.0 if no_pdf else 1.0) * y * pdf)


def unary_call(x, kind, p=1.0):
    xb, yb = Vec(x.numel(), x), Vec(x.numel())
    _lib.call("fqss_unary_fwd", xb.ptr, yb.ptr, x.numel(), kind, p, stream())
    torch.cuda.synchronize()
    assert yb.written() and xb.unchanged()
    return yb.cpu()


@gpu
def test_unary_maps_against_fp64():
    """fqss_unary_fwd / fqss_unary_bwd, kinds 0 - 3 (tanh, sigmoid, x / p, GELU): random normals (with +-0.5 and +-5) against float64;
    at +-0, +-1e-30 and the saturating points +-20, +-100 the exact limits and finiteness, never a relative bound"""
    sp = torch.tensor(SPECIAL)
    body = torch.cat([rnd(4000, seed=1) * 1.5, torch.tensor([0.5, -0.5, 5.0, -5.0])])
    x = torch.cat([sp, body])
    ns = len(SPECIAL)
    gsp = {v: i for i, v in enumerate(SPECIAL) if v != 0.0}
    fails = []
    for kind, name in ((0, "tanh"), (1, "sigmoid"), (2, "div"), (3, "gelu")):
        y = unary_call(x, kind, UN_P)
        ref = unary_ref(x, kind)
        if kind == 2:
            assert bool(torch.equal(_bits(y), _bits(x / np.float32(UN_P)))), "x / p is one IEEE division"
        else:
            measure("unary", name, y[ns:], ref[ns:], unary_ref(body, kind, torch.float32), name, fails)
        s = y[:ns]
        assert bool(torch.isfinite(s).all()), name
        if kind == 0:
            assert s[0] == 0 and s[1] == 0 and bool((s[8:] == torch.tensor([1.0, -1.0, 1.0, -1.0])).all())
            assert abs(float(s[2]) / 1e-30 - 1) <= 1e-6 and abs(float(s[3]) / -1e-30 - 1) <= 1e-6
        elif kind == 1:
            assert bool((s[:4] == 0.5).all()) and float(s[gsp[100.0]]) == 1.0 and 0.0 <= float(s[gsp[-100.0]]) <= 1e-38
            assert abs(float(s[gsp[20.0]]) - 1.0) <= 2.0 ** -23 and 0.0 <= float(s[gsp[-20.0]]) <= 2.1e-9 * (1 + 1e-5)
        elif kind == 3:
            assert s[0] == 0 and s[1] == 0 and float(s[gsp[-100.0]]) == 0.0 and float(s[gsp[100.0]]) == 100.0
            assert float(s[gsp[20.0]]) == 20.0 and abs(float(s[gsp[-20.0]])) <= 1e-30
            assert abs(float(s[2]) / 0.5e-30 - 1) <= 1e-6 and abs(float(s[3]) / -0.5e-30 - 1) <= 1e-6
        # backward: on the fp32 output (kinds 0, 1) or the input (GELU)
        saved = x if kind == 3 else ref.float()
        g = rnd(x.numel(), seed=2 + kind)
        gb, sb, ob = Vec(x.numel(), g), Vec(x.numel(), saved), Vec(x.numel())
        _lib.call("fqss_unary_bwd", gb.ptr, sb.ptr if kind != 2 else None, ob.ptr, x.numel(), kind, UN_P, stream())
        torch.cuda.synchronize()
        assert ob.written() and gb.unchanged() and sb.unchanged()
        gx, gref = ob.cpu(), unary_bwd_ref(g, saved, kind)
        if kind == 2:
            assert bool(torch.equal(_bits(gx), _bits(g / np.float32(UN_P))))
            continue
        b = measure("unary", "d" + name, gx[ns:], gref[ns:], unary_bwd_ref(g[ns:], saved[ns:], kind, torch.float32), "d" + name, fails)
        if kind == 3:
            floor("unary", "dgelu", unary_bwd_ref(g[ns:], saved[ns:], kind, no_pdf=True), gref[ns:], "pdf term dropped", "dgelu", b)
            assert float(gx[gsp[-100.0]]) == 0.0 and float(gx[gsp[100.0]]) == float(g[gsp[100.0]])
            assert float(gx[gsp[20.0]]) == float(g[gsp[20.0]]) and abs(float(gx[gsp[-20.0]])) <= 1e-30
            assert float(gx[0]) == 0.5 * float(g[0]) and float(gx[1]) == 0.5 * float(g[1])
        else:       # tanh' = sigmoid' = 0 where the output saturated to +-1 / 1 / 0 exactly
            for v in (100.0, -100.0) + ((20.0, -20.0) if kind == 0 else ()):
                assert float(gx[gsp[v]]) == 0.0 or (kind == 1 and abs(float(gx[gsp[v]])) <= 1e-37), (name, v)
    assert not fails, fails


@gpu
def test_unary_value_maps_bit_exact():
    """fqss_unary2_fwd kinds 4 - 7: round (half to even), floor, sign, clip(p, p2) bit-exact against torch on .5 ties of both parities,
    negative halves, +-0 and values outside [p, p2]; kinds 0 - 3 through the same entry"""
    x = torch.cat([torch.tensor([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, -3.5, 0.0, -0.0, 0.49999997, -0.49999997, 1e-30, -1e-30,
                                 8388607.5, -8388607.5, 1e10, -1e10, 2.5, -1.25, 2.5000002, -1.2500001]), rnd(2000, seed=3) * 3])
    p, p2 = -1.25, 2.5
    xb = Vec(x.numel(), x)
    want = {4: torch.round(x), 5: torch.floor(x), 6: torch.sign(x), 7: torch.clip(x, p, p2)}
    for kind in (4, 5, 6, 7):
        assert kind == (K.UNARY_ROUND, K.UNARY_FLOOR, K.UNARY_SIGN, K.UNARY_CLIP)[kind - 4]
        yb = Vec(x.numel())
        _lib.call("fqss_unary2_fwd", xb.ptr, yb.ptr, x.numel(), kind, p, p2, stream())
        torch.cuda.synchronize()
        assert yb.written() and xb.unchanged()
        y = yb.cpu()
        assert bool(torch.equal(y, want[kind])), kind
        if kind in (4, 5):
            assert bool(torch.equal(torch.signbit(y), torch.signbit(want[kind]))), "the sign of a zero result"
    half_away = torch.sign(x) * torch.floor(x.abs() + 0.5)                 # roundf
    differs(half_away, want[4].double(), "rintf replaced by roundf", "round")
    yb = Vec(x.numel())
    _lib.call("fqss_unary2_fwd", xb.ptr, yb.ptr, x.numel(), 0, 0.0, 0.0, stream())
    torch.cuda.synchronize()
    assert bool(torch.equal(_bits(yb.cpu()), _bits(unary_call(x, 0))))
    yb = Vec(x.numel())
    _lib.call("fqss_unary2_fwd", xb.ptr, yb.ptr, 0, 4, 0.0, 0.0, stream())
    refused("fqss_unary2_fwd", xb.ptr, yb.ptr, 4, 8, 0.0, 0.0, stream())
    refused("fqss_unary2_fwd", xb.ptr, yb.ptr, 4, -1, 0.0, 0.0, stream())
    refused("fqss_unary2_fwd", None, yb.ptr, 4, 4, 0.0, 0.0, stream())
    refused("fqss_unary_fwd", xb.ptr, yb.ptr, 4, 4, 1.0, stream())
    refused("fqss_unary_fwd", xb.ptr, yb.ptr, -1, 0, 1.0, stream())
    refused("fqss_unary_fwd", xb.ptr, yb.ptr, 4, 2, 0.0, stream())          # division by zero
    refused("fqss_unary_bwd", xb.ptr, xb.ptr, yb.ptr, 4, 4, 1.0, stream())
    refused("fqss_unary_bwd", xb.ptr, None, yb.ptr, 4, 0, 1.0, stream())   # tanh' needs the saved output
    _lib.call("fqss_unary_fwd", xb.ptr, yb.ptr, 0, 0, 1.0, stream())
    _lib.call("fqss_unary_bwd", xb.ptr, xb.ptr, yb.ptr, 0, 0, 1.0, stream())
    torch.cuda.synchronize()
    assert yb.untouched()


@gpu
def test_unary_rows_is_the_flat_map_on_a_column_block():
    """fqss_unary_rows_fwd on a 16-B aligned column block of a wider NaN-padded matrix: bit-identical to fqss_unary_fwd on the dense copy"""
    R, cols, ld = 37, 8, 20
    x = rnd(R, cols, seed=4) * 2
    xb = Blk(R, cols, ld, 4, fill=x)
    for kind in (0, 1, 2, 3):
        yb = Blk(R, cols, cols + 4)
        _lib.call("fqss_unary_rows_fwd", xb.ptr, yb.ptr, R, cols, ld, yb.ld, kind, UN_P, stream())
        torch.cuda.synchronize()
        assert yb.written() and xb.unchanged()
        assert bool(torch.equal(_bits(yb.cpu(R * cols)), _bits(unary_call(x.reshape(-1), kind, UN_P)))), kind
    yb, x1, y1 = Blk(R, cols, cols + 4), Blk(R, cols, ld, 1, fill=x), Blk(R, cols, cols + 4, 1)
    for a in ((xb.ptr, yb.ptr, R, 6, ld, 12), (xb.ptr, yb.ptr, R, cols, ld + 1, 12), (xb.ptr, yb.ptr, R, cols, ld, 13),
              (x1.ptr, yb.ptr, R, cols, ld, 12), (xb.ptr, y1.ptr, R, cols, ld, 12), (xb.ptr, yb.ptr, R, cols, 4, 12),
              (None, yb.ptr, R, cols, ld, 12), (xb.ptr, yb.ptr, -1, cols, ld, 12)):
        refused("fqss_unary_rows_fwd", *a, 0, 1.0, stream())
    refused("fqss_unary_rows_fwd", xb.ptr, yb.ptr, R, cols, ld, 12, 4, 1.0, stream())
    refused("fqss_unary_rows_fwd", xb.ptr, yb.ptr, R, cols, ld, 12, 2, 0.0, stream())
    _lib.call("fqss_unary_rows_fwd", xb.ptr, yb.ptr, 0, cols, ld, 12, 0, 1.0, stream())
    torch.cuda.synchronize()
    assert yb.untouched() and y1.untouched()


@gpu
def test_unary_flat_grid_stride():
    """n = 16384 * 256 + 3: flat_grid is capped at 16384 workgroups and the grid-stride loop of k_unary_fwd runs on"""
    n = 16384 * 256 + 3
    x = rnd(n, seed=6)
    y = unary_call(x, 2, UN_P)
    assert bool(torch.equal(_bits(y), _bits(x / np.float32(UN_P))))


def glu_ref(x, gy, dtype=F64, drop_1ms=False):
    x, gy = x.to(dtype), gy.to(dtype)
    C = x.shape[1] // 2
    a, s = x[:, :C], torch.sigmoid(x[:, C:])
    return {"y": a * s, "ga": gy * s, "gb": gy * a * s * (1.0 if drop_1ms else (1.0 - s))}


@gpu
def test_glu_against_fp64():
    """fqss_glu_fwd / _bwd with ld > M on every tensor: y = a sigmoid(b) and both halves of the gradient"""
    fails = []
    for (B, C, M) in [(1, 1, 1), (2, 3, 77), (3, 24, 130)]:
        tag = f"(B, C, M) = ({B}, {C}, {M})"
        x, gy = rnd(B, 2 * C, M, seed=M) * 2, rnd(B, C, M, seed=M + 1)
        xb, yb = Blk(B * 2 * C, M, M + 3, fill=x), Blk(B * C, M, M + 1)
        _lib.call("fqss_glu_fwd", xb.ptr, yb.ptr, B, C, M, xb.ld, yb.ld, stream())
        gyb, gxb = Blk(B * C, M, M + 2, fill=gy), Blk(B * 2 * C, M, M + 5)
        _lib.call("fqss_glu_bwd", xb.ptr, gyb.ptr, gxb.ptr, B, C, M, xb.ld, gyb.ld, gxb.ld, stream())
        torch.cuda.synchronize()
        assert yb.written() and gxb.written()
        all_unchanged(x=xb, gy=gyb)
        ref, ref32, mut = glu_ref(x, gy), glu_ref(x, gy, torch.float32), glu_ref(x, gy, drop_1ms=True)
        gx = gxb.cpu(B, 2 * C, M)
        measure("glu", "y", yb.cpu(B, C, M), ref["y"], ref32["y"], tag, fails)
        measure("glu", "ga", gx[:, :C], ref["ga"], ref32["ga"], tag, fails)
        b = measure("glu", "gb", gx[:, C:], ref["gb"], ref32["gb"], tag, fails)
        floor("glu", "gb", mut["gb"], ref["gb"], "(1 - s) dropped", tag, b)
    xb, yb = Blk(4, 5, 8, fill=rnd(4, 5)), Blk(4, 5, 8)
    for a in ((-1, 2, 5, 8), (1, 0, 5, 8), (1, 2, 5, 4)):
        refused("fqss_glu_fwd", xb.ptr, yb.ptr, *a, a[3], stream())
        refused("fqss_glu_bwd", xb.ptr, xb.ptr, yb.ptr, *a, a[3], a[3], stream())
    refused("fqss_glu_fwd", None, yb.ptr, 1, 2, 5, 8, 8, stream())
    refused("fqss_glu_bwd", None, xb.ptr, yb.ptr, 1, 2, 5, 8, 8, 8, stream())
    _lib.call("fqss_glu_fwd", xb.ptr, yb.ptr, 0, 2, 5, 8, 8, stream())
    _lib.call("fqss_glu_bwd", xb.ptr, xb.ptr, yb.ptr, 1, 2, 0, 8, 8, 8, stream())
    torch.cuda.synchronize()
    assert yb.untouched()
    assert not fails, fails


@gpu
def test_div_forward_bit_exact_backward_against_fp64():
    """fqss_div_fwd is one IEEE division; fqss_div_bwd: g / b and -g a / b^2 with |b| in [0.1, 3]"""
    fails = []
    for n in (1, 1000):
        a, g = rnd(n, seed=n) * 2, rnd(n, seed=n + 1)
        u = torch.rand(n, generator=torch.Generator().manual_seed(n + 2))
        b = (0.1 + 2.9 * u) * (1 - 2 * (torch.arange(n) % 2))
        ab, bb, gb = Vec(n, a), Vec(n, b), Vec(n, g)
        yb, gab, gbb = Vec(n), Vec(n), Vec(n)
        _lib.call("fqss_div_fwd", ab.ptr, bb.ptr, yb.ptr, n, stream())
        _lib.call("fqss_div_bwd", gb.ptr, ab.ptr, bb.ptr, gab.ptr, gbb.ptr, n, stream())
        torch.cuda.synchronize()
        assert yb.written() and gab.written() and gbb.written()
        all_unchanged(a=ab, b=bb, g=gb)
        assert bool(torch.equal(_bits(yb.cpu()), _bits(a / b)))
        ad, bd, gd = a.double(), b.double(), g.double()
        measure("div", "ga", gab.cpu(), gd / bd, g / b, f"n {n}", fails)
        bnd = measure("div", "gb", gbb.cpu(), -gd * ad / (bd * bd), -g * a / (b * b), f"n {n}", fails)
        floor("div", "gb", -gd * ad / bd, -gd * ad / (bd * bd), "b instead of b^2", f"n {n}", bnd)
    yb = Vec(4)
    refused("fqss_div_fwd", ab.ptr, bb.ptr, yb.ptr, -1, stream())
    refused("fqss_div_fwd", None, bb.ptr, yb.ptr, 4, stream())
    refused("fqss_div_bwd", gb.ptr, ab.ptr, bb.ptr, yb.ptr, yb.ptr, -1, stream())
    refused("fqss_div_bwd", None, ab.ptr, bb.ptr, yb.ptr, yb.ptr, 4, stream())
    _lib.call("fqss_div_fwd", ab.ptr, bb.ptr, yb.ptr, 0, stream())
    torch.cuda.synchronize()
    assert yb.untouched()
    assert not fails, fails


def emb_ref(w, idx, g, dtype=F64):
    """F.embedding with out-of-range rows reading as zeros and adding nothing; gw = the scatter-add of g"""
    V, D = w.shape
    ok = (idx >= 0) & (idx < V)
    out = torch.where(ok[:, None], w.to(dtype)[idx.clamp(0, V - 1)], torch.zeros((), dtype=dtype))
    gw = torch.zeros(V, D, dtype=dtype).index_add_(0, idx[ok], g.to(dtype)[ok])
    return out, gw


def emb_run(w, idx, g, start, gw_ptr=None):
    V, D = w.shape
    n = idx.numel()
    wb, gb, ob = Vec(V * D, w), Vec(n * D, g), Vec(n * D)
    ib = idx.to(DEV)
    ib0 = ib.clone()
    _lib.call("fqss_embedding_fwd", wb.ptr, ib.data_ptr(), ob.ptr, n, D, V, stream())
    gwb = Vec(V * D, start) if gw_ptr is None else None
    _lib.call("fqss_embedding_bwd", gb.ptr, ib.data_ptr(), gwb.ptr if gw_ptr is None else gw_ptr, n, D, V, stream())
    torch.cuda.synchronize()
    assert ob.written() and (gwb is None or gwb.written()) and bool(torch.equal(ib, ib0))
    all_unchanged(w=wb, g=gb)
    return ob.cpu(n, D), None if gwb is None else gwb.cpu(V, D).double() - start.double()


@gpu
def test_embedding_against_fp64():
    """fqss_embedding_fwd (bit-exact gather; rows -1 and V read as zeros) and fqss_embedding_bwd (gw += scatter, gw non-zero on entry;
    duplicates; one case with 5000 indices on one row: fp32 atomics on D addresses)"""
    fails = []
    cases = [(V, D, 50) for V in (1, 7, 100) for D in (1, 3, 64)] + [(7, 3, 5000)]
    for (V, D, n) in cases:
        tag = f"V {V} D {D} n {n}"
        w, g = rnd(V, D, seed=V + D), rnd(n, D, seed=V + D + 1)
        if n == 5000:
            idx = torch.full((n,), 4, dtype=torch.int64)
        else:
            idx = torch.randint(0, V, (n,), generator=torch.Generator().manual_seed(V + D))
            idx[3], idx[17], idx[20], idx[21] = -1, V, idx[5], idx[5]
        out_ref, gw_ref = emb_ref(w, idx, g)
        start = rnd(V, D, seed=9, scale=max(rms(gw_ref), 1e-3))
        out, gw = emb_run(w, idx, g, start)
        exact(out, out_ref, tag)
        b = measure("emb", "gw", gw, gw_ref, emb_ref(w, idx, g, torch.float32)[1], tag, fails)
        hit = torch.zeros(V, dtype=torch.bool)
        hit[idx[(idx >= 0) & (idx < V)]] = True
        assert bool((gw[~hit] == 0).all()), "a row no index names must keep its value"
        drop = g.clone()
        drop[(idx == idx[5]).nonzero()[-1]] = 0                               # the last duplicate of a row lost
        floor("emb", "gw", emb_ref(w, idx, drop)[1], gw_ref, "a duplicate index dropped", tag, b)
    wb, ob = Vec(8, 1.0), Vec(8)
    ib = torch.zeros(4, dtype=torch.int64, device=DEV)
    for a in ((-1, 2, 4), (2, 0, 4), (2, 2, 0)):
        refused("fqss_embedding_fwd", wb.ptr, ib.data_ptr(), ob.ptr, *a, stream())
        refused("fqss_embedding_bwd", wb.ptr, ib.data_ptr(), ob.ptr, *a, stream())
    refused("fqss_embedding_fwd", None, ib.data_ptr(), ob.ptr, 2, 2, 4, stream())
    refused("fqss_embedding_bwd", None, ib.data_ptr(), ob.ptr, 2, 2, 4, stream())
    _lib.call("fqss_embedding_fwd", wb.ptr, ib.data_ptr(), ob.ptr, 0, 2, 4, stream())
    torch.cuda.synchronize()
    assert ob.untouched()
    assert not fails, fails


# =============================================================================================================== deterministic mode
@pytest.fixture
def det_off():
    yield
    if K is not None:
        K.DetMode.off()          # (the control block is device-wide: no later test may run under it)


@gpu
def test_deterministic_gradient_sums_against_fp64(det_off):
    """FQSS_DETERMINISTIC=1 arithmetic (fqss_dev.h grad_add: integer sums on the shadow of the attached slot-0 arena, fqss_det_finish
    rounds once) for k_colsum, the ggamma / gbeta adds of k_gnrows_bwd_reduce and k_embedding_bwd into slices of that arena: two runs are
    bit-identical and both meet the float64 bounds of the atomic path"""
    R1, C1 = 1000, 37
    g1 = rnd(R1, C1, seed=1)
    g1b, ref1 = Blk(R1, C1, C1 + 3, fill=g1), g1.double().sum(0)
    B, C2, Kc, S = 2, 24, 50, 7                                          # 700 rows: 88 workgroups add into every column
    (R2, RB, X), _ = gr_geometry(B, Kc, S, "intra")
    bmap = gr_map(R2, RB, X)
    ops2 = gr_operands(R2, C2, bmap, B, seed=2)
    ref2 = gr_ref(*ops2, GR_EPS, bmap, B)
    V, D, n3 = 7, 3, 5000
    w3, g3 = rnd(V, D, seed=3), rnd(n3, D, seed=4)
    idx3 = torch.randint(0, 2, (n3,), generator=torch.Generator().manual_seed(5)) * 4
    ref3 = emb_ref(w3, idx3, g3)[1]
    arena = torch.zeros(256, device=DEV)
    off = {"cs": 0, "gg": 64, "gb": 128, "gw": 192}
    size = {"cs": C1, "gg": C2, "gb": C2, "gw": V * D}
    slot = {n: arena[off[n]:off[n] + size[n]] for n in off}
    start = {"cs": rnd(C1, seed=8, scale=rms(ref1)), "gg": rnd(C2, seed=9, scale=rms(ref2["ggamma"])),
             "gb": rnd(C2, seed=10, scale=rms(ref2["gbeta"])), "gw": rnd(V * D, seed=11, scale=rms(ref3))}
    det = K.DetMode()
    det.attach(0, arena)
    det.activate()
    runs = []
    for _ in range(2):
        arena.zero_()
        for n, sl in slot.items():
            sl.copy_(start[n])
        _lib.call("fqss_colsum", g1b.ptr, slot["cs"].data_ptr(), R1, C1, g1b.ld, stream())
        got2 = gr_run(ops2, RB, X, B, None, slots=(slot["gg"], slot["gb"]))
        emb_run(w3, idx3, g3, None, gw_ptr=slot["gw"].data_ptr())
        det.finish(0)
        torch.cuda.synchronize()
        runs.append(arena.cpu().clone())
    K.DetMode.off()
    assert bool(torch.equal(runs[0], runs[1])), "deterministic mode: the sums of two runs differ"
    a = runs[0]
    gaps = torch.ones_like(a, dtype=torch.bool)
    for n in off:
        gaps[off[n]:off[n] + size[n]] = False
    assert bool((a[gaps] == 0).all()), "a write between the gradient slots"
    add = {n: a[off[n]:off[n] + size[n]].double() - start[n].double() for n in off}
    fails = []
    measure("colsum", "out", add["cs"], ref1, None, "deterministic k_colsum", fails)
    measure("gnrows", "ggamma", add["gg"], ref2["ggamma"], None, "deterministic k_gnrows_bwd_reduce", fails)
    measure("gnrows", "gbeta", add["gb"], ref2["gbeta"], None, "deterministic k_gnrows_bwd_reduce", fails)
    measure("gnrows", "gx", got2["gx"], ref2["gx"], None, "deterministic mode, gx", fails)
    measure("emb", "gw", add["gw"].reshape(V, D), ref3, None, "deterministic k_embedding_bwd", fails)
    assert not fails, fails


# ==================================================================================================== the references, without a GPU
def _spec_hop(x, nfft, hop):
    """_ref_spec of test_gpu_kernels.py (hop = nfft / 4), generalised to a hop: torch.stft of the re-padded signal, frames 2 .. 2 + le"""
    if hop * 4 == nfft:
        return _ref_spec(x, nfft)
    le, pad = -(-x.shape[-1] // hop), hop // 2 * 3
    xp = F.pad(x, (pad, pad + le * hop - x.shape[-1]), mode="reflect")
    z = torch.stft(xp, nfft, hop, window=torch.hann_window(nfft).to(x.dtype), win_length=nfft, normalized=True, center=True, return_complex=True,
                   pad_mode="reflect")[..., :-1, :]
    return z[..., 2:2 + le]


def _ispec_hop(z, nfft, hop, length):
    """_ref_ispec of test_gpu_kernels.py, generalised to a hop and with the window in the spectrum's precision (with its fp32 window
    torch.istft forms the envelope in fp32 and the float64 tie would stop at 1e-8)"""
    z = F.pad(F.pad(z, (0, 0, 0, 1)), (2, 2))
    pad = hop // 2 * 3
    le = hop * -(-length // hop) + 2 * pad
    x = torch.istft(z, nfft, hop, window=torch.hann_window(nfft).to(z.real.dtype), win_length=nfft, normalized=True, length=le, center=True)
    return x[..., pad:pad + length]


def test_references_on_cpu():
    """The formula references of this file in float64 against torch's own stft / istft (through _ref_spec / _ref_ispec of
    test_gpu_kernels.py, generalised to a hop) and the autograd of the inverse, the emulated fft_lds against torch.fft, the dual-path
    index formulas against oracle.dptnet_oracle, the gLN closed form against F.group_norm and its autograd.  Needs no device."""
    tight = lambda a, b, tol=1e-11: float((a.double() - b.double()).abs().max()) <= tol * max(1.0, float(b.double().abs().max()))     # noqa: E731
    for N in SPEC_N:
        v = torch.complex(rnd(2, N, seed=N).double(), rnd(2, N, seed=N + 1).double())
        assert tight(torch.view_as_real(fft_emul(v)), torch.view_as_real(torch.fft.fft(v)), 1e-12)
        assert tight(torch.view_as_real(fft_emul(v, True) / N), torch.view_as_real(torch.fft.ifft(v)), 1e-12)
        for mut in ("r2tail", "r4tw"):
            void = (N.bit_length() - 1) % 3 != (1 if mut == "r2tail" else 2)
            assert tight(torch.view_as_real(fft_emul(v, mut=mut)), torch.view_as_real(torch.fft.fft(v)), 1e-12) == void
        for hop in (N // 4, N // 2):
            pad = hop // 2 * 3
            for L in (2 * N + 3, 5 * hop, spec_shortest_L(N, hop, pad)):
                T = -(-L // hop)
                x, zin, g = rnd(2, L, seed=L).double(), rnd(2, 2, T, N // 2, seed=L + 1).double(), rnd(2, L, seed=L + 2).double()
                ours = stft_ref(x, N, hop, T, pad)
                right = (T - 1) * hop + N - 1 - pad - (L - 1)
                if max(pad, right) < L and hop * 4 == N and pad + T * hop - L < L:      # (torch refuses a reflection as long as the signal)
                    want = _spec_hop(x, N, hop).transpose(-1, -2)
                    assert tight(ours[:, 0], want.real) and tight(ours[:, 1], want.imag), (N, hop, L)
                if max(pad, right) < L:
                    # the header's own formula for any hop: frames at f hop - pad of the reflect-padded signal
                    xp = F.pad(x, (pad, max(right, 0)), mode="reflect")
                    if xp.shape[-1] >= (T - 1) * hop + N:
                        want = torch.stft(xp, N, hop, window=hann(N), normalized=True, center=False, return_complex=True)[..., :-1, :T].transpose(-1, -2)
                        assert tight(ours[:, 0], want.real) and tight(ours[:, 1], want.imag), (N, hop, L)
                zc = torch.complex(zin[:, 0], zin[:, 1]).transpose(-1, -2).clone().requires_grad_(True)
                yt = _ispec_hop(zc, N, hop, L)
                assert tight(istft_ref(zin, N, hop, pad, L), yt.detach(), 1e-10), (N, hop, L)
                yt.backward(g)
                gz = istft_bwd_ref(g, N, hop, pad, T)
                assert tight(gz[:, 0], zc.grad.real.transpose(-1, -2), 1e-10) and tight(gz[:, 1], zc.grad.imag.transpose(-1, -2), 1e-10), (N, hop, L)
                assert abs(float((istft_ref(zin, N, hop, pad, L) * g).sum() - (zin * gz).sum() + (zin[:, 1, :, 0] * gz[:, 1, :, 0]).sum())) <= 1e-9 * L
    # with hop = N the periodic Hann envelope has a zero
    assert float(envelope(64, 64).min()) == 0.0 and float(envelope(64, 32).min()) >= 0.5 - 1e-12
    # dual-path chunking: dp_chunks arithmetic, the segment formula and the merge formula against the oracle
    for Kc in (2, 4, 10):
        for T in dp_T_list(Kc):
            rest, S = chunks_ref(T, Kc)
            P = Kc // 2
            assert (rest, S) == (Kc - (P + T % Kc) % Kc, 2 * (T + rest + P) // Kc) and (S // 2) * Kc >= T + P
            f = rnd(3, 5, T, seed=T).double()
            want, _ = segment_ref(f, torch.zeros(Kc, 3 * S, 5), Kc)
            assert bool(torch.equal(segment_formula(f, Kc, S), want)), (Kc, T)
            for nspk in (1, 2, 3):
                o = merge_operand(S, 2, Kc, nspk, 5, seed=T).double()
                x4 = o.reshape(S, 2, Kc, nspk, 5).permute(1, 3, 4, 2, 0).reshape(2 * nspk, 5, Kc, S)
                a, b = DO.merge_halves(x4)
                fa, fb = merge_formula(o, 2, nspk, 5, Kc, S)
                assert bool(torch.equal(fa, a)) and bool(torch.equal(fb, b)), (Kc, T, nspk)
                if hasattr(DO, "merge_feature"):
                    m = DO.merge_feature(x4, rest)
                    assert bool(torch.equal((fa + fb)[..., :m.shape[-1]], m))
    assert any(chunks_ref(T, 10)[0] == 10 for T in dp_T_list(10)) and any(T < 5 for T in dp_T_list(10))
    # gLN closed form against F.group_norm in float64, both layouts; the other layout's map is a different map
    for layout in ("intra", "inter"):
        (R, RB, X), (_, RBo, Xo) = gr_geometry(2, 3, 5, layout)
        bmap = gr_map(R, RB, X)
        assert not bool(torch.equal(bmap, gr_map(R, RBo, Xo)))
        assert bool(torch.equal(bmap, torch.arange(R) // X % 2))          # (r % RB) / X = r / X % B whenever RB = B X
        ops = gr_operands(R, 8, bmap, 2, seed=1)
        ref, tor = gr_ref(*ops, 1e-5, bmap, 2), gr_torch(*ops, 1e-5, bmap, 2, F64)
        for n in ("y", "mean", "rstd", "gx", "ggamma", "gbeta"):
            assert tight(ref[n], tor[n]), (layout, n)
    # the element-wise references against autograd
    x = (rnd(200, seed=1) * 2).double().requires_grad_(True)
    g = rnd(200, seed=2).double()
    gelu = F.gelu(x)
    assert tight(unary_ref(x.detach(), 3), gelu.detach())
    assert tight(unary_bwd_ref(g, x.detach(), 3), torch.autograd.grad(gelu, x, g)[0])
    for kind, fn in ((0, torch.tanh), (1, torch.sigmoid)):
        y = fn(x)
        assert tight(unary_bwd_ref(g, y.detach(), kind), torch.autograd.grad(y, x, g)[0])
    xx, gy = rnd(2, 6, 9, seed=3).double().requires_grad_(True), rnd(2, 3, 9, seed=4).double()
    y = F.glu(xx, 1)
    ref = glu_ref(xx.detach(), gy)
    gxx, = torch.autograd.grad(y, xx, gy)
    assert tight(ref["y"], y.detach()) and tight(ref["ga"], gxx[:, :3]) and tight(ref["gb"], gxx[:, 3:])
    w = rnd(7, 3, seed=5).double().requires_grad_(True)
    idx = torch.tensor([0, 3, 3, 6, 1, 3])
    out = F.embedding(idx, w)
    gg = rnd(6, 3, seed=6).double()
    o_ref, gw_ref = emb_ref(w.detach(), idx, gg)
    assert tight(o_ref, out.detach()) and tight(gw_ref, torch.autograd.grad(out, w, gg)[0])
