"""The channel-first float streaming kernels at kernel level against float64: GroupNorm(1, C) and its quantizing pair, the forward-only
GroupNorm tails, the depthwise convolution (csrc/stream_ops.hip), BatchNorm (csrc/batchnorm.hip, ops_dp.BatchNormFn), the per-sample
normalisation and LayerScale kernels (csrc/hd_ops.hip) and the HTDemucs loss (csrc/hd_loss.hip).  The C entry points are called through
fqss_amd._lib with explicit pointers and leading dimensions, so alignment and ld -- which choose the kernel instance -- are fixed per case.

Entry points covered: fqss_gn_fwd, fqss_gn_bwd, fqss_gnq_fwd_f, fqss_gnq_bwd_f, fqss_gn_fwd_tail, fqss_dwconv_fwd, fqss_dwconv_bwd_x,
fqss_dwconv_bwd_w, fqss_bn_moments, fqss_bn_apply, fqss_bn_bwd_reduce, fqss_bn_bwd_apply (and ops_dp.BatchNormFn under BatchNormQ),
fqss_sample_meanstd, fqss_sample_norm, fqss_chan_op, fqss_chan_scale_bwd, fqss_col_scale_fwd, fqss_col_scale_bwd, fqss_hd_kd_loss, and
the deterministic-mode form of the three fp32 gradient atomics (k_dwconv_bwd_w, k_chan_scale_bwd, k_gn_bwd_coef with nbs > 1).

Measured on the MI355X: largest e_elem / e_norm over the well-conditioned cases of a family (|mean| / std = 0.3), beside torch fp32 on
the CPU on the same cases, the bound (BOUND below) and its factor over the measurement (largest of two runs where atomics make runs differ):
                                         kernel               fp32                 bound                factor
  GroupNorm (fqss_gn_fwd / fqss_gn_bwd)
    y                                    5.2e-7 / 2.4e-7      5.2e-7 / 6.1e-8      1.6e-6 / 8e-7        3.1 / 3.3   (e_norm: the one element of (1,1,1))
    rstd                                 5.9e-8 / 5.4e-8      1.0e-7 / 6.3e-8      2e-7 / 2e-7          3.4 / 3.7
    gx                                   4.4e-7 / 4.7e-8      5.9e-7 / 6.5e-8      1.5e-6 / 1.6e-7      3.4 / 3.4   ((1,1,1), zero reference: 9.2e-8 of gz gamma rstd)
    ggamma, gbeta                        3.0e-7 / 1.0e-7, 2.8e-7 / 6.4e-8   fp32 1.0e-6 / 8.4e-7, 1.5e-6 / 1.5e-6   1e-6 / 3.5e-7, 1e-6 / 2.2e-7   3.3 .. 3.6
    mean, per unit of std                <= 1.5e-8 (offset 30: 8.7e-7, 1000: 8.5e-6)       (|mean| / std + 1) 2^-24: one rounding to fp32
  quantizing pair (fqss_gnq_fwd_f / fqss_gnq_bwd_f), range [-2.5, 2.7]: about 2 % clipped at each end
    codes one level off                  1 of 49 200, 0 of 20 495, 0 of 2 142, 3 of 240 000  (torch fp32: the same counts); cap 2e-4
    y on equal codes                     5.2e-7               -                    1.6e-6               3.1
    gx                                   6.6e-7 / 6.5e-8      8.0e-7 / 6.5e-8      2.2e-6 / 2.2e-7      3.3 / 3.4
    ggamma, gbeta                        3.5e-7 / 7.6e-8, 2.6e-7 / 7.1e-8   fp32 9.4e-7 / 5.0e-7, 8.9e-7 / 5.9e-7   1.2e-6 / 2.6e-7, 9e-7 / 2.4e-7   3.4
    range gradients (relative)           1.65e-6 (min), 1.8e-6 (max) without a code off; fp32 1.6e-5, 8.9e-7      6e-6      3.3 .. 3.6
                                         with codes off: 7.3e-4 / 2.3e-4 (a), 2.3e-5 / 3.6e-5 (e) = the |g| / 255 per such element that the test allows
  tails (fqss_gn_fwd_tail)               gelu 7.5e-7 / 5.7e-8, glu 3.9e-7 / 4.0e-8   fp32 the same to two digits   2.5e-6 / 2e-7, 1.3e-6 / 1.4e-7   3.3 .. 3.5
  depthwise convolution
    z, gx                                5.1e-7 / 5.1e-8, 5.1e-7 / 5.4e-8   fp32 5.1e-7 / 5.1e-8, 4.9e-7 / 6.1e-8   1.7e-6 / 1.7e-7, 1.7e-6 / 1.8e-7   3.3
    gw (fp32 atomics, deterministic too) 3.2e-7 / 1.1e-7      9.0e-7 / 4.0e-7      1.1e-6 / 3.6e-7      3.4 / 3.2
  BatchNorm entries
    sum, sum g                           0 (exact in fp64 at these sizes)          4e-15 (the float64 reference's own rounding; fp32: 4.3e-7, 9.7e-7)
    sum x^2, sum g x                     1.0e-15 / 8.8e-16, 1.4e-15 / 8.3e-16 (also at |mean| / std = 1000)   4e-15     2.9 .. 4.0
    y, gx (fqss_bn_apply / _bwd_apply)   4.6e-7 / 2.6e-8, 4.0e-7 / 3.3e-8   fp32 3.2e-7 / 3.8e-8, 5.2e-7 / 4.7e-8   1.6e-6 / 1e-7, 1.4e-6 / 1.2e-7   3.5 .. 3.8
  BatchNormFn / BatchNormQ               y 2.7e-7 / 4.4e-8, gx 2.5e-7 / 4.2e-8, gamma 7.5e-8 / 4.6e-8, beta 5.9e-8 / 3.3e-8, running mean 1.2e-7 / 7.5e-8,
                                         running var 7.0e-8 / 4.8e-8   (fp32: 3.3e-7, 4.8e-7, 2.5e-7, 1.7e-7, 8.8e-8, 9.8e-8)   bounds 3.0 .. 3.6 x
  per-sample normalisation               fp64 moments (ws) 2.7e-16 / 2.1e-16, 0 at |mean| / std = 1000 (fp32 9.4e-8 / 5.1e-8)   1e-15 = 3.7 x
                                         std 4.8e-8 / 3.6e-8, forward 4.1e-7 / 5.4e-8, inverse 3.3e-7 / 3.7e-8, round trip 7.1e-7 / 5.1e-8
                                         (fp32: 4.8e-8, 3.9e-7, 3.3e-7, 4.9e-7)   bounds 3.3 .. 3.5 x;  mean per unit of std <= 2.4e-8 (offset 1000: 3.3e-5)
  LayerScale, channel-first              y 2.2e-7 / 2.8e-8, gx 2.4e-7 / 2.5e-8 (= fp32), gs 4.3e-7 / 2.3e-7 (fp32 4.6e-7 / 1.2e-7)   bounds 3.2 .. 3.6 x
  LayerScale, channel-last               y 2.3e-7 / 2.7e-8, gx 2.3e-7 / 2.5e-8 (= fp32), gs 2.1e-6 / 1.1e-6 (fp32 3.9e-7 / 1.8e-7: up to 1025 fp32 atomics
                                         per column on top of 32-row serial sums; it differs run to run)   bounds 3.3 .. 3.7 x, gs 7e-6 / 3.2e-6 = 3.3 / 2.9 x
  fqss_hd_kd_loss                        loss 1.0e-7, task 4.6e-8 / 2.5e-8, kd 5.4e-7 / 3.6e-7, w 9.0e-7 / 4.0e-7, gradient 9.7e-7 / 4.0e-7
                                         (fp32: 1.3e-7, 9.7e-8, 1.7e-7, 9.0e-7, 8.3e-7)   bounds 2.5e-7, 1.6e-7 / 1e-7, 1.4e-6, 3e-6 / 1.4e-6, 3.5e-6 / 1.5e-6 = 2.5 .. 4.0 x
Offset cases (bound = COND = 4 x torch fp32's own error on the case; measured kernel / fp32 ratio): GroupNorm y 0.67 (offset 30), 0.96 (1000;
4.8e-5 against 5.0e-5), gx 0.29 / 0.02, ggamma 0.04; BatchNormFn y 1.66 (5.1e-5 against 3.1e-5), gx 0.28; per-sample forward 1.00; the loss
gradient at N = 1 (every w from single-sample SDRs): 1.69.

Mutation floors (smallest e_elem a wrong kernel gives over the cases where it is not void; each bound is asserted 10 x below, per case):
last column slice dropped from the statistics: y 0.22, tails 0.58; last sample slice dropped from ggamma / gbeta: 1.7 / 1.2; mean rounded
to bf16: y 8.3e-5 (52 x the bound), tails 3.9e-4, per-sample forward 6.7e-4; eps omitted, case g: 8.8e-2 at (1,1,64), not finite at
(1,1,1); STE omitted: gx 4.4; outermost tap dropped: z 1.1, gx 1.6, gw 0.97; padding column M read as 1.0: z 0.57; biased std at n = 50:
1.1e-2; sgn(0) = +1: gradient 2.5e-3 (lambda 1), 0.11, 1.9; the 1e-7 of new_sdr omitted on the silent source: w is not finite; a dropped
last sample: BatchNorm sum x^2 3.6e-3.  Void by construction and skipped: tap and padding mutations at K = 1 and at dil 128 / M 100
(no outer tap lands), mean -> bf16 at a single element, column / sample slices where the launch has one.

Layout under test.  Operands sit in NaN-filled flat buffers between guard floats, row padding [M, ld) stays NaN (a read of it poisons the
result); outputs are NaN-filled buffers.  After each call: guards and everything outside an output's rows still NaN, every element [0, M)
of an output finite, every operand bit-identical to what was uploaded.  Output padding columns may be written (the kernels say so).

References: plain float64 torch on the CPU (closed forms below; test_references_on_cpu checks them against torch's own float64 group_norm /
batch_norm / conv autograd and oracle.fqss_oracle).  e_elem = max |got - ref| / rms(ref), e_norm = ||got - ref|| / ||ref||; the yardstick
is the same operation in torch fp32 on the CPU, printed beside every kernel figure ("MEAS" lines)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import oracle.fqss_oracle as O

K = None
_lib = None
DEV = "cuda"
NAN = float("nan")
EINVAL = -22
G = 64                                   # guard floats on either side of every buffer
F64 = torch.float64

# ---------------------------------------------------------------------------------------------------------------------------- bounds
# per family and tensor: (e_elem bound, e_norm bound), at most 4 x the largest figure measured on the MI355X over the family's
# well-conditioned cases (see the table above); the offset cases take COND x the fp32 yardstick's own error on the same case
BOUND = {
    "gn": {"y": (1.6e-6, 8e-7), "rstd": (2e-7, 2e-7), "gx": (1.5e-6, 1.6e-7), "ggamma": (1e-6, 3.5e-7), "gbeta": (1e-6, 2.2e-7)},
    "gnq": {"y": (1.6e-6, 0.0), "rstd": (2e-7, 1e-7), "gx": (2.2e-6, 2.2e-7), "ggamma": (1.2e-6, 2.6e-7), "gbeta": (9e-7, 2.4e-7),
            "glo": (6e-6, 0.0), "ghi": (6e-6, 0.0)},      # (y: on the elements whose code agrees; glo / ghi: relative error of the scalar)
    "tail": {"gelu": (2.5e-6, 2e-7), "glu": (1.3e-6, 1.4e-7)},
    "dw": {"z": (1.7e-6, 1.7e-7), "gx": (1.7e-6, 1.8e-7), "gw": (1.1e-6, 3.6e-7)},
    "bn": {"sum": (4e-15, 4e-15), "sumsq": (4e-15, 4e-15), "sg": (4e-15, 4e-15), "sgx": (4e-15, 4e-15), "y": (1.6e-6, 1e-7), "gx": (1.4e-6, 1.2e-7)},
    "bnfn": {"y": (8e-7, 1.5e-7), "gx": (9e-7, 1.5e-7), "gw": (2.5e-7, 1.5e-7), "gb": (2e-7, 1.1e-7), "rm": (4e-7, 2.5e-7), "rv": (2.4e-7, 1.6e-7)},
    "sample": {"moments": (1e-15, 1e-15), "std": (1.6e-7, 1.2e-7), "norm": (1.4e-6, 1.8e-7), "inv": (1.1e-6, 1.3e-7), "trip": (2.4e-6, 1.7e-7)},
    "chan": {"y": (7.5e-7, 1e-7), "gx": (8e-7, 9e-8), "gs": (1.5e-6, 7.5e-7)},
    "col": {"y": (7.5e-7, 1e-7), "gx": (8e-7, 9e-8), "gs": (7e-6, 3.2e-6)},
    "loss": {"loss": (2.5e-7, 2.5e-7), "task": (1.6e-7, 1e-7), "kd": (1.4e-6, 1.4e-6), "w": (3e-6, 1.4e-6), "grad": (3.5e-6, 1.5e-6)},
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
        return float("inf"), float("inf")
    d = a - ref
    return float(d.abs().max() / rms(ref)), float(d.norm() / ref.norm())


def stream():
    return torch.cuda.current_stream().cuda_stream


def refused(name, *args):
    """the entry returns FQSS_EINVAL and fqss_last_error names it"""
    rc = _lib._bind(name)(*args)
    msg = _lib.load().fqss_last_error().decode()
    torch.cuda.synchronize()
    assert rc == EINVAL and name in msg, (name, rc, msg)
    return msg


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


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
        self.ptr = self.buf.data_ptr() + 4 * self.o
        self.before = None
        if fill is not None:
            self.view.copy_(fill.reshape(R, M))
            self.before = self.buf.clone()

    def vec(self):
        return self.ptr % 16 == 0 and self.ld % 4 == 0

    def unchanged(self):
        return bool(torch.equal(_bits(self.buf), _bits(self.before)))

    def written(self):
        """[0, M) of every row finite; everything outside the R rows of ld floats still NaN (padding columns may be written)"""
        end = self.o + self.R * self.ld
        return (bool(torch.isfinite(self.view).all()) and bool(torch.isnan(self.buf[:self.o]).all()) and bool(torch.isnan(self.buf[end:]).all()))

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
    f_elem, f_norm = errs(ref32, ref) if ref32 is not None else (float("nan"), float("nan"))
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


# ====================================================================================================================== GroupNorm(1, C)
def gn_slices(row_wgs, M, vec):
    """gn_col_slices of csrc/stream_ops.hip: grid.z of k_gn_stats / k_gn_bwd_rows"""
    if row_wgs >= 512:
        return 1
    return max(1, min(1024 // max(row_wgs, 1), -(-M // (256 * vec * 4)), 65535))


def gn_nbs(B):
    """sample slices of k_gn_bwd_coef's parameter-gradient blocks (gn_bwd_impl)"""
    return 1 if B <= 16 else min(64, -(-B // 16))


def gn_moments(x, drop_slice=None):
    """per-sample (mean, biased variance) of x [B, C, M] in float64; drop_slice = (vec, zs): the wrong kernel whose last column slice
    (columns m with (m // (256 vec)) % zs == zs - 1) never reaches the sums, which are still divided by C M"""
    B, C, M = x.shape
    x = x.double()
    if drop_slice is not None:
        vec, zs = drop_slice
        keep = ((torch.arange(M) // (256 * vec)) % zs != zs - 1).double()
        x = x * keep
    n = C * M
    mean = x.sum((1, 2)) / n
    var = ((x * x).sum((1, 2)) / n - mean * mean).clamp_(min=0.0)
    return mean, var


def fq_ref(pre, lo, hi):
    """the 8-bit asymmetric quantizer in float64 -> (y, codes, in-range mask, u): qat_quant.py's arithmetic, STE on the rounding"""
    delta = (hi - lo) / 255.0
    u = (pre - lo) / delta
    X = torch.round(u)
    inr = (X >= 0) & (X <= 255)
    c = X.clamp(0, 255)
    return delta * c + lo, c, inr, u


def gn_ref(x, gz, gamma, beta, eps, q=None, mean=None, var=None, no_eps=False, drop_samples=0):
    """GroupNorm(1, C) of x [B, C, M] and its backward for the output gradient gz in closed form, float64.  q = (lo, hi): the output is
    fq(GroupNorm(x)), gz is the gradient of the quantized output, the STE zeroes it outside the range and glo / ghi are the range
    gradients.  mean / var: statistics of a wrong kernel; no_eps: eps left out of rstd; drop_samples: the last n samples left out of
    ggamma / gbeta"""
    B, C, M = x.shape
    x, gz, gamma, beta = x.double(), gz.double(), gamma.double(), beta.double()
    if mean is None:
        mean, var = gn_moments(x)
    rstd = 1.0 / torch.sqrt(var + (0.0 if no_eps else eps))
    xh = (x - mean[:, None, None]) * rstd[:, None, None]
    pre = xh * gamma[None, :, None] + beta[None, :, None]
    out = {"mean": mean, "rstd": rstd, "pre": pre, "y": pre}
    g = gz
    if q is not None:
        lo, hi = (torch.tensor(float(np.float32(v)), dtype=F64) for v in q)
        y, c, inr, u = fq_ref(pre, lo, hi)
        ghi = (gz * torch.where(inr, c - u, c)).sum() / 255.0
        out.update(y=y, codes=c.to(torch.uint8), glo=(gz * (~inr)).sum() - ghi, ghi=ghi, inr=inr, u=u)
        g = gz * inr
    Bk = B - drop_samples
    out["gbeta"] = g[:Bk].sum((0, 2))
    out["ggamma"] = (g[:Bk] * xh[:Bk]).sum((0, 2))
    gh = g * gamma[None, :, None]
    out["gx"] = rstd[:, None, None] * (gh - gh.mean((1, 2), keepdim=True) - xh * (gh * xh).mean((1, 2), keepdim=True))
    return out


def gn_torch(x, gz, gamma, beta, eps, dtype, q=None):
    """the same through torch's own group_norm and autograd (and the oracle's quantizer) in `dtype`: the fp32 yardstick; in float64 the
    check of gn_ref"""
    X, ga, be = (t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
    pre = F.group_norm(X, 1, ga, be, eps)
    out = {"pre": pre.detach()}
    y = pre
    if q is not None:
        lo, hi = (torch.tensor([float(np.float32(v))], dtype=dtype, requires_grad=True) for v in q)
        y = O.act_quantize(pre, lo, hi)
        out["codes"] = O.act_indices(pre.detach(), lo.detach(), hi.detach())
    y.backward(gz.to(dtype))
    xd = X.detach().reshape(x.shape[0], -1)
    out.update(y=y.detach(), gx=X.grad, ggamma=ga.grad, gbeta=be.grad, mean=xd.mean(1), rstd=1.0 / torch.sqrt(xd.var(1, unbiased=False) + eps))
    if q is not None:
        out.update(glo=lo.grad[0], ghi=hi.grad[0])
    return out


def gn_operands(B, C, M, seed, offset=0.3, scale=1.0, const=None):
    """x = scale (randn + offset) (|mean| / std = offset), or the constant `const`; gz ~ N(0, 1); gamma ~ 1.3 (1 +- 0.1), beta ~ 0.2 +- 0.1:
    the normalised output is about 1.3 randn + 0.2"""
    x = torch.full((B, C, M), const) if const is not None else (rnd(B, C, M, seed=seed) + offset) * scale
    return x, rnd(B, C, M, seed=seed + 1), 1.3 * (1 + 0.1 * rnd(C, seed=seed + 2)), 0.2 + 0.1 * rnd(C, seed=seed + 3)


QRANGE = (-2.5, 2.7)                     # clips about 2 % of 1.3 randn + 0.2 at each end
GN_EPS = 1e-5


class GnRun:
    """one forward and backward of fqss_gn_fwd / fqss_gn_bwd (q: fqss_gnq_fwd_f / fqss_gnq_bwd_f) with every tensor in a buffer of its own.
    lay: {"x" | "gz" | "y" | "gx": (ld, off)}; start: the values ggamma / gbeta hold before the call (they are added to); slots: views of
    a deterministic-mode arena to take the parameter gradients instead"""

    def __init__(self, ops, lay, eps=GN_EPS, q=None, codes=False):
        x, gz, gamma, beta = ops
        self.B, self.C, self.M = B, C, M = x.shape
        self.eps, self.q = eps, q
        R = B * C
        self.x, self.gz = Blk(R, M, *lay["x"], fill=x), Blk(R, M, *lay["gz"], fill=gz)
        self.y, self.gx = Blk(R, M, *lay["y"]), Blk(R, M, *lay["gx"])
        self.gamma, self.beta = Vec(C, gamma), Vec(C, beta)
        self.mr = Vec(2 * B)
        self.yc = None
        if q is not None:
            self.qmin, self.qmax = Vec(1, torch.tensor([q[0]])), Vec(1, torch.tensor([q[1]]))
            if codes:
                self.ld_yc = (M + 3) // 4 * 4 + 4
                self.yc = torch.full((G + R * self.ld_yc + G,), 0xEE, dtype=torch.uint8, device=DEV)

    def paths(self):
        """the launch path by the thresholds of gn_fwd_impl / gn_bwd_impl, as the case ids spell it"""
        B, C, M = self.B, self.C, self.M
        vs = 4 if self.x.vec() else 1
        va = 4 if self.x.vec() and self.y.vec() else 1
        vb = 4 if self.gz.vec() and self.x.vec() else 1
        vg = 4 if vb == 4 and self.gx.vec() else 1
        return (f"stats VEC{vs} x{gn_slices(min(C, 64) * B, M, vs)}, apply VEC{va}, rows VEC{vb} x{gn_slices(C * B, M, vb)}, "
                f"bwd apply VEC{vg}, nbs {gn_nbs(B)}")

    def stats_path(self):
        vs = 4 if self.x.vec() else 1
        return vs, gn_slices(min(self.C, 64) * self.B, self.M, vs)

    def forward(self):
        B, C, M = self.B, self.C, self.M
        ws = Vec(2 * B, dtype=F64)
        if self.q is None:
            _lib.call("fqss_gn_fwd", self.x.ptr, self.gamma.ptr, self.beta.ptr, self.y.ptr, self.mr.ptr, B, C, M, self.x.ld, self.y.ld,
                      self.eps, ws.ptr, stream())
        else:
            _lib.call("fqss_gnq_fwd_f", self.x.ptr, self.gamma.ptr, self.beta.ptr, self.y.ptr, None if self.yc is None else self.yc.data_ptr() + G,
                      self.mr.ptr, B, C, M, self.x.ld, self.y.ld, 0 if self.yc is None else self.ld_yc, self.eps, ws.ptr, self.qmin.ptr,
                      self.qmax.ptr, stream())
        torch.cuda.synchronize()
        assert self.y.written(), "y: a NaN inside the rows or a write outside them"
        assert self.mr.written() and ws.guards() and self.gx.untouched()
        all_unchanged(x=self.x, gz=self.gz, gamma=self.gamma, beta=self.beta)
        if self.yc is not None:
            assert bool((self.yc[:G] == 0xEE).all()) and bool((self.yc[-G:] == 0xEE).all()), "a write outside the code rows"
        return self

    def codes(self):
        R = self.B * self.C
        return self.yc[G:G + R * self.ld_yc].view(R, self.ld_yc)[:, :self.M].cpu().reshape(self.B, self.C, self.M)

    def backward(self, start, slots=None):
        B, C, M = self.B, self.C, self.M
        ws = Vec(2 * B * C + 2 * B, dtype=F64)
        if slots is None:
            self.gg, self.gb = Vec(C, start[0]), Vec(C, start[1])
            pg, pb = self.gg.ptr, self.gb.ptr
        else:
            pg, pb = slots[0].data_ptr(), slots[1].data_ptr()
        mr_before = self.mr.buf.clone()
        if self.q is None:
            _lib.call("fqss_gn_bwd", self.gz.ptr, self.x.ptr, self.gamma.ptr, self.mr.ptr, self.gx.ptr, pg, pb, B, C, M, self.gz.ld, self.x.ld,
                      self.gx.ld, ws.ptr, stream())
        else:
            self.gacc = torch.zeros(K.GACC_DOUBLES, dtype=F64, device=DEV)
            _lib.call("fqss_gnq_bwd_f", self.gz.ptr, self.x.ptr, self.gamma.ptr, self.beta.ptr, self.mr.ptr, self.gx.ptr, pg, pb, B, C, M,
                      self.gz.ld, self.x.ld, self.gx.ld, ws.ptr, self.qmin.ptr, self.qmax.ptr, self.gacc.data_ptr(), stream())
        torch.cuda.synchronize()
        assert self.gx.written(), "gx: a NaN inside the rows or a write outside them"
        assert ws.guards() and bool(torch.equal(_bits(self.mr.buf), _bits(mr_before))), "the backward wrote outside ws or changed mean_rstd"
        if slots is None:
            assert self.gg.written() and self.gb.written()
        all_unchanged(x=self.x, gz=self.gz, gamma=self.gamma, beta=self.beta)
        return self

    def range_grads(self):
        """the range partials through K.gacc_flush into fp32 gradients that start non-zero"""
        gmin, gmax = torch.full((1,), 0.25, device=DEV), torch.full((1,), -0.5, device=DEV)
        K.gacc_flush(self.gacc, gmin, gmax, None)
        torch.cuda.synchronize()
        assert float(self.gacc.abs().max()) == 0.0
        return float(gmin) - 0.25, float(gmax) + 0.5

    def outputs(self, start=None):
        B, C, M = self.B, self.C, self.M
        mr = self.mr.cpu(B, 2)
        out = {"y": self.y.cpu(B, C, M), "mean": mr[:, 0], "rstd": mr[:, 1], "gx": self.gx.cpu(B, C, M)}
        if start is not None:
            out.update(ggamma=self.gg.cpu().double() - start[0].double(), gbeta=self.gb.cpu().double() - start[1].double())
        return out


def gn_layout(M, kind):
    """-> {"x" | "gz" | "y" | "gx": (ld, off)}.  "pad": 16-B aligned rows with NaN padding; "dense": ld = M; "x+1" / "gz+1" / "out+1":
    padded rows (ld % 4 == 0) with that tensor's base one float (4 B) past a 16-B boundary"""
    ld = M if kind == "dense" else pad4(M)
    lay = {n: (ld, 0) for n in ("x", "gz", "y", "gx")}
    if kind == "x+1":
        lay["x"] = (ld, 1)
    elif kind == "gz+1":
        lay["gz"] = (ld, 1)
    elif kind == "out+1":
        lay["y"], lay["gx"] = (ld, 1), (ld, 1)
    else:
        assert kind in ("pad", "dense")
    return lay


# id = "<case of the issue> | <launch path>" -> (B, C, M), layout, operand options.  The path is GnRun.paths(): it restates
#   gn_fwd_impl:  VEC 4 iff x is 16-B aligned with ld % 4 == 0 (apply: and y); grid.z = gn_col_slices(min(C, 64) B, M, VEC)
#   gn_bwd_impl:  VEC 4 iff gz and x are (apply: and gx); grid.z = gn_col_slices(C B, M, VEC); nbs = 1 for B <= 16, else min(64, cdiv(B, 16))
#   gn_col_slices(w, M, VEC) = 1 for w >= 512, else min(1024 / w, cdiv(M, 1024 VEC)): > 1 needs M > 4096 (VEC 4) or M > 1024 (VEC 1)
# and is asserted against the id, so a moved threshold names the case to move.
GN_CASES = {
    "a (2,3,8200) padded 16-B rows | stats VEC4 x3, apply VEC4, rows VEC4 x3, bwd apply VEC4, nbs 1": ((2, 3, 8200), "pad", {}),
    "b (1,5,4099) dense rows, M % 4 = 3 | stats VEC1 x5, apply VEC1, rows VEC1 x5, bwd apply VEC1, nbs 1": ((1, 5, 4099), "dense", {}),
    "c (2,3,8200) x 4 B off | stats VEC1 x9, apply VEC1, rows VEC1 x9, bwd apply VEC1, nbs 1": ((2, 3, 8200), "x+1", {}),
    "c (2,3,8200) gz 4 B off | stats VEC4 x3, apply VEC4, rows VEC1 x9, bwd apply VEC1, nbs 1": ((2, 3, 8200), "gz+1", {}),
    "c (2,3,8200) y and gx 4 B off | stats VEC4 x3, apply VEC1, rows VEC4 x3, bwd apply VEC1, nbs 1": ((2, 3, 8200), "out+1", {}),
    "d (17,6,21) sample slices of 9 and 8 | stats VEC4 x1, apply VEC4, rows VEC4 x1, bwd apply VEC4, nbs 2": ((17, 6, 21), "pad", {}),
    "e (40,300,20) two channel blocks | stats VEC4 x1, apply VEC4, rows VEC4 x1, bwd apply VEC4, nbs 3": ((40, 300, 20), "pad", {}),
    "f (3,70,130) channel loop past 64 | stats VEC4 x1, apply VEC4, rows VEC4 x1, bwd apply VEC4, nbs 1": ((3, 70, 130), "pad", {}),
    "g (1,1,1) | stats VEC4 x1, apply VEC4, rows VEC4 x1, bwd apply VEC4, nbs 1": ((1, 1, 1), "pad", {"scale": 0.01}),
    "g (1,1,64) | stats VEC4 x1, apply VEC4, rows VEC4 x1, bwd apply VEC4, nbs 1": ((1, 1, 64), "pad", {"scale": 0.01}),
    "i (2,3,8200) mean / std 30 | stats VEC4 x3, apply VEC4, rows VEC4 x3, bwd apply VEC4, nbs 1": ((2, 3, 8200), "pad", {"offset": 30.0}),
    "i (2,3,8200) mean / std 1000 | stats VEC4 x3, apply VEC4, rows VEC4 x3, bwd apply VEC4, nbs 1": ((2, 3, 8200), "pad", {"offset": 1000.0}),
}


def gn_start(C, ref):
    """non-zero starting values of ggamma / gbeta, of the sums' own size"""
    return rnd(C, seed=41, scale=max(rms(ref["ggamma"]), 1e-3)), rnd(C, seed=42, scale=max(rms(ref["gbeta"]), 1e-3))


def gn_floors(tag, fam, ops, ref, stats_path, eps, q, bounds):
    """what the wrong kernels of the issue give on this case's operands, each at least 10 x above the bound in force.
    stats_path = (VEC, column slices) of the statistics launch"""
    x, gz, gamma, beta = ops
    B, C, M = x.shape
    vs, zs = stats_path
    if zs > 1:
        m_mean, m_var = gn_moments(x, drop_slice=(vs, zs))
        mut = gn_ref(x, gz, gamma, beta, eps, q, mean=m_mean, var=m_var)
        floor(fam, "y", mut["pre"], ref["pre"], "last column slice dropped from the statistics", tag, bounds["y"])
    nbs = gn_nbs(B)
    if nbs > 1:
        per = -(-B // nbs)
        mut = gn_ref(x, gz, gamma, beta, eps, q, drop_samples=B - (nbs - 1) * per)
        for n in ("ggamma", "gbeta"):
            floor(fam, n, mut[n], ref[n], "last sample slice dropped", tag, bounds[n])
    if B * C * M > 1:                # (void at one element: the mean is the element, and bf16(x) - x times rstd is no rounding error of a mean)
        mut = gn_ref(x, gz, gamma, beta, eps, q, mean=ref["mean"].bfloat16().double(), var=gn_moments(x)[1])
        floor(fam, "y", mut["pre"], ref["pre"], "mean rounded to bf16", tag, bounds["y"])
    if tag.startswith("g "):
        mut = gn_ref(x, gz, gamma, beta, eps, q, no_eps=True)
        floor(fam, "y", mut["pre"], ref["pre"], "eps omitted", tag, bounds["y"])


@gpu
@pytest.mark.parametrize("case", list(GN_CASES))
def test_groupnorm_against_fp64(case):
    """fqss_gn_fwd / fqss_gn_bwd: y, mean_rstd, gx and the sums ADDED into ggamma / gbeta (non-zero on entry) against float64.  The mean is
    rounded once to fp32: |mean| 2^-24 is its bound; the offset cases bound y and the gradients by COND x torch fp32's own error."""
    (B, C, M), kind, opt = GN_CASES[case]
    ops = gn_operands(B, C, M, seed=500 + M + B, **opt)
    offset = opt.get("offset", 0.3)
    cond = offset > 1.0
    run = GnRun(ops, gn_layout(M, kind))
    assert case.split(" | ")[1] == run.paths(), run.paths()
    ref = gn_ref(*ops, GN_EPS)
    # (torch's group_norm refuses a single value per channel: at one element the yardstick is the float64 result rounded to fp32)
    ref32 = gn_torch(*ops, GN_EPS, torch.float32) if B * C * M > 1 else {n: t.float() for n, t in ref.items()}
    start = gn_start(C, ref)
    got = run.forward().backward(start).outputs(start)
    fails, bounds = [], {}
    mean_err = float(((got["mean"].double() - ref["mean"]) * ref["rstd"]).abs().max())
    mean_bound = (float((ref["mean"].abs() * ref["rstd"]).max()) + 1.0) * MEAN_ULP
    print(f"MEAS gn mean |d mean| / std {mean_err:.2e} bound {mean_bound:.2e} | {case}")
    if not mean_err <= mean_bound:
        fails.append((case, "mean", mean_err, mean_bound))
    measure("gn", "rstd", got["rstd"], ref["rstd"], ref32["rstd"], case, fails)
    for n in ("y", "gx", "ggamma", "gbeta"):
        r = ref[n]
        if n == "gx" and B * C * M == 1:
            # one element: y = beta whatever x is and gx = gz c1 + c3 cancels to zero: |gx| against the size of the terms that cancel
            e = float(got[n].abs().max()) / (abs(float(ops[1])) * float(ref["rstd"]) * abs(float(ops[2])))
            print(f"MEAS gn gx zero-ref {e:.2e} | {case}")
            if not e <= BOUND["gn"]["gx"][0]:
                fails.append((case, "gx zero reference", e))
            continue
        if n == "ggamma" and B * M == 1:
            continue                 # (xhat = 0: the reference is exactly 0 and so is ds - db mean)
        bounds[n] = measure("gn", n, got[n], r, ref32[n], case, fails, cond=cond and n != "gbeta")
    assert not fails, fails
    gn_floors(case, "gn", ops, ref, run.stats_path(), GN_EPS, None, bounds)


@gpu
def test_groupnorm_constant_input():
    """case h: a constant input at (2,3,8200), three column slices: E[x^2] - mean^2 cancels to rounding noise (clamped at 0 when negative),
    rstd = 1 / sqrt(eps) and every output stays finite; y = beta up to the one rounding of shift = beta - scale mean (|scale mean| 2^-23)"""
    B, C, M = 2, 3, 8200
    ops = gn_operands(B, C, M, seed=77, const=0.7)
    run = GnRun(ops, gn_layout(M, "pad"))
    ref = gn_ref(*ops, GN_EPS)
    start = gn_start(C, ref)
    got = run.forward().backward(start).outputs(start)
    for n, t in got.items():
        assert bool(torch.isfinite(t).all()), n
    c = float(np.float32(0.7))
    assert bool((got["mean"] == c).all())
    rstd0 = 1.0 / math.sqrt(GN_EPS)
    e = float((got["rstd"].double() / rstd0 - 1).abs().max())
    print(f"MEAS gn constant input: rstd relative {e:.2e}, y - beta {float((got['y'].double() - ops[3].double()[None, :, None]).abs().max()):.2e}")
    assert e <= 1e-6          # (var + eps with |var| <= 2^-52 x^2 sqrt(n) rounding noise against eps = 1e-5, then one fp32 rounding)
    scale = rstd0 * float(ops[2].abs().max())
    assert float((got["y"].double() - ops[3].double()[None, :, None]).abs().max()) <= 2.0 ** -23 * scale * c * 1.5
    assert errs(got["gbeta"], ref["gbeta"])[0] <= BOUND["gn"]["gbeta"][0]


GNQ_CASES = [c for c in GN_CASES if c[0] in "abde"]


@gpu
@pytest.mark.parametrize("with_codes", [True, False], ids=["yc", "no yc"])
@pytest.mark.parametrize("case", GNQ_CASES)
def test_groupnorm_quantizing_pair(case, with_codes):
    """fqss_gnq_fwd_f / fqss_gnq_bwd_f on a range that clips about 2 % at each end: codes against act_indices of the float64 GroupNorm (no
    code more than one level off, at most 2e-4 of them one level off), y = the de-quantised code, gx / ggamma / gbeta against the float64
    STE, the range gradients through gacc and K.gacc_flush.  A code one level off moves a range gradient by |g| / 255: that much is
    allowed on top of the bound per such element."""
    (B, C, M), kind, opt = GN_CASES[case]
    ops = gn_operands(B, C, M, seed=600 + M + B, **opt)
    run = GnRun(ops, gn_layout(M, kind), q=QRANGE, codes=with_codes)
    assert case.split(" | ")[1] == run.paths(), run.paths()
    ref, ref32 = gn_ref(*ops, GN_EPS, q=QRANGE), gn_torch(*ops, GN_EPS, torch.float32, q=QRANGE)
    clipped = 1.0 - float(ref["inr"].double().mean())
    assert 0.01 <= clipped <= 0.08, clipped
    start = gn_start(C, ref)
    got = run.forward().backward(start).outputs(start)
    glo, ghi = run.range_grads()
    fails, bounds = [], {}
    lo, hi = (float(np.float32(v)) for v in QRANGE)
    delta = (hi - lo) / 255.0
    code_of_y = torch.round((got["y"].double() - lo) / delta)
    dc = (code_of_y - ref["codes"].double()).abs()
    if with_codes:
        assert bool(torch.equal(run.codes().double(), code_of_y)), "the code output is not the code of y"
    nflip = int((dc != 0).sum())
    f32flip = int((ref32["codes"].double() != ref["codes"].double()).sum())
    print(f"MEAS gnq codes one level off: {nflip} of {dc.numel()} (torch fp32: {f32flip}) | {case}")
    assert float(dc.max()) <= 1.0 and nflip <= 2e-4 * dc.numel(), (nflip, float(dc.max()))
    same = dc == 0
    y_err = float((got["y"].double() - ref["y"])[same].abs().max()) / rms(ref["y"])
    print(f"MEAS gnq y e_elem on equal codes {y_err:.2e} | {case}")
    if not y_err <= BOUND["gnq"]["y"][0]:
        fails.append((case, "y", y_err))
    measure("gnq", "rstd", got["rstd"], ref["rstd"], ref32["rstd"], case, fails)
    for n in ("gx", "ggamma", "gbeta"):
        bounds[n] = measure("gnq", n, got[n], ref[n], ref32[n], case, fails)
    flip_allow = float(ops[1].double()[~same].abs().sum()) / 255.0
    for n, v in (("glo", glo), ("ghi", ghi)):
        r = float(ref[n])
        e, e32 = abs(v - r), abs(float(ref32[n]) - r)
        b = BOUND["gnq"][n][0] * abs(r) + flip_allow
        print(f"MEAS gnq {n} rel {e / abs(r):.2e} fp32 {e32 / abs(r):.2e} (value {r:.4g}, flip allowance {flip_allow / abs(r):.1e}) | {case}")
        if not e <= b:
            fails.append((case, n, e, b))
    assert not fails, fails
    nbs = gn_nbs(B)
    if nbs > 1:
        mut = gn_ref(*ops, GN_EPS, QRANGE, drop_samples=B - (nbs - 1) * (-(-B // nbs)))
        for n in ("ggamma", "gbeta"):
            floor("gnq", n, mut[n], ref[n], "last sample slice dropped", case, bounds[n])
    # the STE left out (gz passed where the output clipped): what the bound on gx must exclude
    mut = gn_ref(*ops, GN_EPS)
    floor("gnq", "gx", mut["gx"], ref["gx"], "STE omitted", case, bounds["gx"])


# ================================================================================================================= fqss_gn_fwd_tail
def tail_ref(x, gamma, beta, eps, tail, ls, res, dtype=F64, mean_bf16=False, drop_slice=None):
    """tail 1: gelu(gn(x)) (erf form); tail 2: glu(gn(x)) * ls[c] + res"""
    if dtype == F64:
        mean, var = gn_moments(x, drop_slice)
        if mean_bf16:
            mean = mean.bfloat16().double()
        g = gn_ref(x, torch.zeros_like(x), gamma, beta, eps, mean=mean, var=var)["pre"]
    else:
        g = F.group_norm(x.to(dtype), 1, gamma.to(dtype), beta.to(dtype), eps)
    if tail == 1:
        return 0.5 * g * (1.0 + torch.erf(g * (1.0 / math.sqrt(2.0))))
    Co = x.shape[1] // 2
    return g[:, :Co] * torch.sigmoid(g[:, Co:]) * ls.to(dtype)[None, :, None] + res.to(dtype)


# id -> (B, C, M), residual layout.  x and y always sit on padded 16-B rows (the entry demands it); statistics grid.z =
# gn_col_slices(min(C, 64) B, M, 4); res_vec = 1 iff the residual is 16-B aligned with ld % 4 == 0 and ld >= round-up(M, 4)
TAIL_CASES = {
    "(2,6,8200) 3 column slices, padded residual (res_vec 1)": ((2, 6, 8200), "pad", 3),
    "(1,4,4099) 2 column slices, dense residual [1,2,4099] (res_vec 0: last group read clamped)": ((1, 4, 4099), "dense", 2),
    "(1,4,4099) 2 column slices, padded residual (res_vec 1)": ((1, 4, 4099), "pad", 2),
    "(5,24,77) 1 slice, dense residual (res_vec 0)": ((5, 24, 77), "dense", 1),
    "(5,24,77) 1 slice, padded residual (res_vec 1)": ((5, 24, 77), "pad", 1),
}


@gpu
@pytest.mark.parametrize("case", list(TAIL_CASES))
def test_groupnorm_tails_against_fp64(case):
    """fqss_gn_fwd_tail, tail 1 (GELU) and tail 2 (GLU * LayerScale + residual), against float64"""
    (B, C, M), res_kind, zs = TAIL_CASES[case]
    assert zs == gn_slices(min(C, 64) * B, M, 4)
    x, _, gamma, beta = gn_operands(B, C, M, seed=700 + M)
    Co = C // 2
    ls, res = 0.5 + 0.2 * rnd(Co, seed=3), rnd(B, Co, M, seed=4)
    fails = []
    for tail, name in ((1, "gelu"), (2, "glu")):
        ref = tail_ref(x, gamma, beta, GN_EPS, tail, ls, res)
        ref32 = tail_ref(x, gamma, beta, GN_EPS, tail, ls, res, dtype=torch.float32)
        xb, gb, bb = Blk(B * C, M, pad4(M), fill=x), Vec(C, gamma), Vec(C, beta)
        Cy = C if tail == 1 else Co
        yb = Blk(B * Cy, M, pad4(M))
        lsb = Vec(Co, ls)
        rb = Blk(B * Co, M, M if res_kind == "dense" else pad4(M), fill=res)
        assert rb.vec() == ("res_vec 1" in case)
        ws = Vec(2 * B, dtype=F64)
        _lib.call("fqss_gn_fwd_tail", xb.ptr, gb.ptr, bb.ptr, yb.ptr, B, C, M, xb.ld, yb.ld, GN_EPS, ws.ptr, tail, lsb.ptr if tail == 2 else None,
                  rb.ptr if tail == 2 else None, rb.ld if tail == 2 else 0, stream())
        torch.cuda.synchronize()
        assert yb.written() and ws.guards()
        all_unchanged(x=xb, gamma=gb, beta=bb, ls=lsb, res=rb)
        measure("tail", name, yb.cpu(B, Cy, M), ref, ref32, f"{case}, tail {tail}", fails)
        floor("tail", name, tail_ref(x, gamma, beta, GN_EPS, tail, ls, res, mean_bf16=True), ref, "mean rounded to bf16", case)
        if zs > 1:
            floor("tail", name, tail_ref(x, gamma, beta, GN_EPS, tail, ls, res, drop_slice=(4, zs)), ref, "last column slice dropped", case)
    assert not fails, fails


@gpu
def test_groupnorm_tail_refuses_bad_arguments():
    """odd C for tail 2, x or y off 16-B alignment or with ld % 4 != 0, a null ls or res, an unknown tail: FQSS_EINVAL, nothing written"""
    B, C, M = 2, 6, 40
    x, _, gamma, beta = gn_operands(B, C, M, seed=1)
    xb, x1, gb, bb = Blk(B * C, M, 44, fill=x), Blk(B * C, M, 44, 1, fill=x), Vec(C, gamma), Vec(C, beta)
    xo = Blk(B * C, M, 43, fill=x)
    yb, y1 = Blk(B * C, M, 44), Blk(B * C, M, 44, 1)
    lsb, rb, ws = Vec(C // 2, 1.0), Blk(B * C // 2, M, 44, fill=rnd(B, C // 2, M)), Vec(2 * B, dtype=F64)

    def args(x=xb, y=yb, C=C, tail=2, ls=lsb.ptr, res=rb.ptr):
        return (x.ptr, gb.ptr, bb.ptr, y.ptr, B, C, M, x.ld, y.ld, GN_EPS, ws.ptr, tail, ls, res, rb.ld, stream())
    refused("fqss_gn_fwd_tail", *args(C=5))
    refused("fqss_gn_fwd_tail", *args(x=x1))
    refused("fqss_gn_fwd_tail", *args(x=x1, tail=1))
    refused("fqss_gn_fwd_tail", *args(x=xo, tail=1))
    refused("fqss_gn_fwd_tail", *args(y=y1))
    refused("fqss_gn_fwd_tail", *args(y=y1, tail=1))
    refused("fqss_gn_fwd_tail", *args(ls=None))
    refused("fqss_gn_fwd_tail", *args(res=None))
    refused("fqss_gn_fwd_tail", *args(tail=3))
    assert yb.untouched() and y1.untouched() and ws.untouched()


# ============================================================================================================= depthwise convolution
def dw_ref(x, w, bias, gz, dil, pad, dtype=F64, drop_tap=False, pad_col_one=False):
    """depthwise 'same' cross-correlation and its gradients by autograd.  drop_tap: the outermost tap (k = K - 1) ignored; pad_col_one:
    the first padding column x[M] read as 1.0 instead of masked"""
    B, C, M = x.shape
    X, W = x.to(dtype).clone().requires_grad_(True), w.to(dtype).clone().requires_grad_(True)
    Wk = W
    if drop_tap:
        Wk = W * torch.cat([torch.ones(w.shape[1] - 1, dtype=dtype), torch.zeros(1, dtype=dtype)])
    xin = torch.cat([X, torch.ones(B, C, 1, dtype=dtype)], 2) if pad_col_one else X
    z = F.conv1d(xin, Wk[:, None, :], None if bias is None else bias.to(dtype), padding=pad, dilation=dil, groups=C)[..., :M]
    z.backward(gz.to(dtype))
    return {"z": z.detach(), "gx": X.grad, "gw": W.grad}


# (K, dil, pad) by id; every one is a 'same' convolution (2 pad = dil (K - 1)).  k_dwconv_v4 loads a tap as one float4 iff its offset
# k dil - pad is a multiple of 4 (and the four floats lie inside the row's ld), and masks columns >= M by hand
DW_TAPS = {
    "K 1": (1, 1, 0),
    "K 2, dil 2": (2, 2, 1),
    "K 3, dil 1": (3, 1, 1),
    "K 3, dil 128 at M 100: only the centre tap lands": (3, 128, 128),
    "K 5, dil 3": (5, 3, 6),
    "K 8, dil 4: no tap offset a multiple of 4": (8, 4, 14),
    "K 8, dil 8: every tap offset a multiple of 4": (8, 8, 28),
}
# layout -> (M, ld of (M), offset of x / gz, offset of the outputs): the v4 kernel needs every base 16-B aligned and ld % 4 == 0
DW_LAYOUTS = {
    "v4, M 100": (100, pad4, 0, 0), "v4, M 130": (130, pad4, 0, 0), "v4, M 131": (131, pad4, 0, 0),
    "scalar, dense M 131": (131, lambda M: M, 0, 0), "scalar, x 4 B off, M 130": (130, pad4, 1, 0), "scalar, outputs 4 B off, M 100": (100, pad4, 0, 1),
}


@gpu
@pytest.mark.parametrize("taps", list(DW_TAPS))
def test_dwconv_against_fp64(taps):
    """fqss_dwconv_fwd (with and without bias), fqss_dwconv_bwd_x and fqss_dwconv_bwd_w (gw non-zero on entry: it accumulates) at C = 7,
    B = 3 on every layout of DW_LAYOUTS against float64 conv1d(groups = C) autograd"""
    Kt, dil, pad = DW_TAPS[taps]
    assert 2 * pad == dil * (Kt - 1)
    B, C = 3, 7
    fails = []
    for lname, (M, ldf, off_in, off_out) in DW_LAYOUTS.items():
        if dil == 128 and M != 100:
            continue
        tag = f"{taps}; {lname}"
        ld = ldf(M)
        x, gz, w, bias = rnd(B, C, M, seed=M + Kt), rnd(B, C, M, seed=M + Kt + 1), rnd(C, Kt, seed=Kt, scale=0.5), rnd(C, seed=9)
        ref, ref32 = dw_ref(x, w, bias, gz, dil, pad), dw_ref(x, w, bias, gz, dil, pad, dtype=torch.float32)
        xb, gzb, wb, bb = Blk(B * C, M, ld, off_in, fill=x), Blk(B * C, M, ld, off_in, fill=gz), Vec(C * Kt, w), Vec(C, bias)
        zb, z0, gxb = Blk(B * C, M, ld, off_out), Blk(B * C, M, ld, off_out), Blk(B * C, M, ld, off_out)
        assert (xb.vec() and zb.vec()) == lname.startswith("v4")
        start = rnd(C, Kt, seed=5, scale=rms(ref["gw"]))
        gwb = Vec(C * Kt, start)
        st = stream()
        _lib.call("fqss_dwconv_fwd", xb.ptr, wb.ptr, bb.ptr, zb.ptr, B, C, M, Kt, dil, pad, xb.ld, zb.ld, st)
        _lib.call("fqss_dwconv_fwd", xb.ptr, wb.ptr, None, z0.ptr, B, C, M, Kt, dil, pad, xb.ld, z0.ld, st)
        _lib.call("fqss_dwconv_bwd_x", gzb.ptr, wb.ptr, gxb.ptr, B, C, M, Kt, dil, pad, gzb.ld, gxb.ld, st)
        _lib.call("fqss_dwconv_bwd_w", gzb.ptr, xb.ptr, gwb.ptr, B, C, M, Kt, dil, pad, gzb.ld, xb.ld, st)
        torch.cuda.synchronize()
        assert zb.written() and z0.written() and gxb.written() and gwb.written(), tag
        all_unchanged(x=xb, gz=gzb, w=wb, bias=bb)
        got = {"z": zb.cpu(B, C, M), "gx": gxb.cpu(B, C, M), "gw": gwb.cpu(C, Kt).double() - start.double()}
        for n in got:
            measure("dw", n, got[n], ref[n], ref32[n], tag, fails)
        nb = errs(z0.cpu(B, C, M), ref["z"] - bias.double()[None, :, None])[0]
        if not nb <= BOUND["dw"]["z"][0]:
            fails.append((tag, "z without bias", nb))
        # floors; void by construction: K = 1 has no outer tap and reaches no padding column; at dil 128 / M 100 no outer tap lands
        if Kt > 1 and dil != 128:
            mut = dw_ref(x, w, bias, gz, dil, pad, drop_tap=True)
            for n in ("z", "gx", "gw"):
                floor("dw", n, mut[n], ref[n], "outermost tap dropped", tag)
            mut = dw_ref(x, w, bias, gz, dil, pad, pad_col_one=True)
            floor("dw", "z", mut["z"], ref["z"], "padding column M read as 1.0", tag)
    assert not fails, fails


@gpu
def test_dwconv_refuses_bad_arguments():
    """K = 9 (kMaxTaps = 8) on all three entries; 2 pad != dil (K - 1) on the forward and the input gradient: FQSS_EINVAL, nothing written"""
    B, C, M = 2, 3, 40
    xb, gzb, wb = Blk(B * C, M, 44, fill=rnd(B, C, M)), Blk(B * C, M, 44, fill=rnd(B, C, M, seed=1)), Vec(C * 9, rnd(C, 9))
    zb, gwb = Blk(B * C, M, 44), Vec(C * 9)
    st = stream()
    refused("fqss_dwconv_fwd", xb.ptr, wb.ptr, None, zb.ptr, B, C, M, 9, 1, 4, 44, 44, st)
    refused("fqss_dwconv_bwd_x", gzb.ptr, wb.ptr, zb.ptr, B, C, M, 9, 1, 4, 44, 44, st)
    refused("fqss_dwconv_bwd_w", gzb.ptr, xb.ptr, gwb.ptr, B, C, M, 9, 1, 4, 44, 44, st)
    for Kt, dil, pad in ((3, 1, 0), (3, 2, 1), (2, 1, 1), (4, 1, 1)):
        refused("fqss_dwconv_fwd", xb.ptr, wb.ptr, None, zb.ptr, B, C, M, Kt, dil, pad, 44, 44, st)
        refused("fqss_dwconv_bwd_x", gzb.ptr, wb.ptr, zb.ptr, B, C, M, Kt, dil, pad, 44, 44, st)
    assert zb.untouched() and gwb.untouched()


# ======================================================================================================================== BatchNorm
def bn_grid(B, C):
    """bn_reduce_grid of csrc/batchnorm.hip -> grid.y (batch slices; each walks b = y, y + gy, ...)"""
    gy = 1
    while gy < B and C * gy < 1024:
        gy *= 2
    return min(gy, B)


# id -> (B, C, M), expected grid.y of the reductions, |mean| / std of x
BN_CASES = {
    "(5,1,77): gy 8 clamped to B = 5": ((5, 1, 77), 5, 0.3),
    "(3,700,33): gy 2, batch loop with a one-sample last pass": ((3, 700, 33), 2, 0.3),
    "(2,1100,9): gy 1, batch loop": ((2, 1100, 9), 1, 0.3),
    "(300,3,5): gy 512 clamped to B = 300": ((300, 3, 5), 300, 0.3),
    "(1,2,70001): column grid capped at 64": ((1, 2, 70001), 1, 0.3),
    "(5,4,77) mean / std 1000": ((5, 4, 77), 5, 1000.0),
}


@gpu
@pytest.mark.parametrize("case", list(BN_CASES))
def test_batchnorm_entries_against_fp64(case):
    """fqss_bn_moments / fqss_bn_bwd_reduce (fp64 sums, atomics into zeroed [C][2]) and the two affine passes fqss_bn_apply /
    fqss_bn_bwd_apply with given coefficients, every tensor on padded NaN rows of its own stride"""
    (B, C, M), gy, offset = BN_CASES[case]
    assert gy == bn_grid(B, C)
    if "capped" in case:
        assert -(-M // 1024) > 64
    x, g = (rnd(B, C, M, seed=800 + M) + offset) * 0.7, rnd(B, C, M, seed=801 + M)
    a, b, c3 = 1 + 0.3 * rnd(C, seed=1), 0.3 * rnd(C, seed=2), 0.3 * rnd(C, seed=3)
    xb, gb = Blk(B * C, M, M + 3, fill=x), Blk(B * C, M, M + 1, 1, fill=g)
    ab, bb, cb = Vec(C, a), Vec(C, b), Vec(C, c3)
    mom, red = Vec(2 * C, 0.0, F64), Vec(2 * C, 0.0, F64)
    yb, gxb = Blk(B * C, M, M + 2), Blk(B * C, M, M + 5, 1)
    st = stream()
    _lib.call("fqss_bn_moments", xb.ptr, mom.ptr, B, C, M, xb.ld, st)
    _lib.call("fqss_bn_bwd_reduce", gb.ptr, xb.ptr, red.ptr, B, C, M, gb.ld, xb.ld, st)
    _lib.call("fqss_bn_apply", xb.ptr, ab.ptr, bb.ptr, yb.ptr, B, C, M, xb.ld, yb.ld, st)
    _lib.call("fqss_bn_bwd_apply", gb.ptr, xb.ptr, ab.ptr, bb.ptr, cb.ptr, gxb.ptr, B, C, M, gb.ld, xb.ld, gxb.ld, st)
    torch.cuda.synchronize()
    assert mom.written() and red.written() and yb.written() and gxb.written()
    all_unchanged(x=xb, g=gb, a=ab, b=bb, c3=cb)
    xd, gd, ad, bd, cd = (t.double() for t in (x, g, a, b, c3))
    x32, g32 = x.float(), g.float()
    bc = lambda v: v[None, :, None]      # noqa: E731
    ref = {"sum": xd.sum((0, 2)), "sumsq": (xd * xd).sum((0, 2)), "sg": gd.sum((0, 2)), "sgx": (gd * xd).sum((0, 2)),
           "y": xd * bc(ad) + bc(bd), "gx": gd * bc(ad) + xd * bc(bd) + bc(cd)}
    ref32 = {"sum": x32.sum((0, 2)), "sumsq": (x32 * x32).sum((0, 2)), "sg": g32.sum((0, 2)), "sgx": (g32 * x32).sum((0, 2)),
             "y": x32 * bc(a) + bc(b), "gx": g32 * bc(a) + x32 * bc(b) + bc(c3)}
    m, r = mom.cpu(C, 2), red.cpu(C, 2)
    got = {"sum": m[:, 0], "sumsq": m[:, 1], "sg": r[:, 0], "sgx": r[:, 1], "y": yb.cpu(B, C, M), "gx": gxb.cpu(B, C, M)}
    fails = []
    for n in got:
        measure("bn", n, got[n], ref[n], ref32[n], case, fails)
    assert not fails, fails
    # a wrong kernel that drops the last batch slice's last sample: the moment bounds are far below it
    if B > 1:
        floor("bn", "sumsq", (xd[:-1] * xd[:-1]).sum((0, 2)), ref["sumsq"], "last sample dropped", case)


@gpu
def test_batchnorm_row_limit():
    """B C = 65535 rows at M = 1 run (grid.y of the affine passes); B C = 65536 is refused by both affine entries with nothing written"""
    for B, C in ((65535, 1), (1, 65535), (257, 255)):
        x, g = rnd(B, C, 1, seed=B), rnd(B, C, 1, seed=B + 1)
        a, b, c3 = rnd(C, seed=1), rnd(C, seed=2), rnd(C, seed=3)
        xb, gb, ab, bb, cb = Blk(B * C, 1, fill=x), Blk(B * C, 1, fill=g), Vec(C, a), Vec(C, b), Vec(C, c3)
        yb, gxb = Blk(B * C, 1), Blk(B * C, 1)
        _lib.call("fqss_bn_apply", xb.ptr, ab.ptr, bb.ptr, yb.ptr, B, C, 1, 1, 1, stream())
        _lib.call("fqss_bn_bwd_apply", gb.ptr, xb.ptr, ab.ptr, bb.ptr, cb.ptr, gxb.ptr, B, C, 1, 1, 1, 1, stream())
        torch.cuda.synchronize()
        assert yb.written() and gxb.written()
        fails = []
        measure("bn", "y", yb.cpu(B, C, 1), x.double() * a.double()[None, :, None] + b.double()[None, :, None], None, f"B C = {B} x {C}", fails)
        measure("bn", "gx", gxb.cpu(B, C, 1), g.double() * a.double()[None, :, None] + x.double() * b.double()[None, :, None]
                + c3.double()[None, :, None], None, f"B C = {B} x {C}", fails)
        assert not fails, fails
    B, C = 65536, 1
    xb, ab, yb = Blk(B * C, 1, fill=rnd(B, C, 1)), Vec(C, 1.0), Blk(B * C, 1)
    refused("fqss_bn_apply", xb.ptr, ab.ptr, ab.ptr, yb.ptr, B, C, 1, 1, 1, stream())
    refused("fqss_bn_bwd_apply", xb.ptr, xb.ptr, ab.ptr, ab.ptr, ab.ptr, yb.ptr, B, C, 1, 1, 1, 1, stream())
    refused("fqss_bn_apply", xb.ptr, ab.ptr, ab.ptr, yb.ptr, 256, 256, 1, 1, 1, stream())
    assert yb.untouched()


# id -> (form, input shape, module options, mode, number of calls)
BNFN_CASES = {
    "1-d [B,C,M], train": ("1d", (6, 5, 33), {}, "train", 1),
    "1-d [B,C], train": ("1d", (16, 5), {}, "train", 1),
    "2-d [B,C,H,W], train, momentum 0.3, eps 1e-3": ("2d", (3, 4, 5, 7), {"momentum": 0.3, "eps": 1e-3}, "train", 1),
    "1-d [B,C,M], eval: running statistics, c2 = c3 = 0": ("1d", (6, 5, 33), {}, "eval", 1),
    "2-d [B,C,H,W], eval": ("2d", (3, 4, 5, 7), {}, "eval", 1),
    "1-d, affine=False, train": ("1d", (6, 5, 33), {"affine": False}, "train", 1),
    "1-d, affine=False, eval": ("1d", (6, 5, 33), {"affine": False}, "eval", 1),
    "1-d, momentum=None over three calls": ("1d", (6, 5, 33), {"momentum": None}, "train", 3),
    "1-d, track_running_stats=False, train": ("1d", (6, 5, 33), {"track_running_stats": False}, "train", 1),
    "1-d, track_running_stats=False, eval: batch statistics": ("1d", (6, 5, 33), {"track_running_stats": False}, "eval", 1),
    "1-d [B,C,M], train, mean / std 1000": ("1d", (6, 5, 33), {}, "train", 1),
}


@gpu
@pytest.mark.parametrize("case", list(BNFN_CASES))
def test_batchnorm_layer_against_fp64(case):
    """BatchNormQ without a quantizer (act_quant=False: the float module; ops_dp.BatchNormFn on csrc/batchnorm.hip with its C-sized host
    arithmetic) against nn.BatchNorm1d / 2d in float64 on the CPU: output, input gradient, gamma / beta gradients, running mean and
    variance, num_batches_tracked after every call"""
    from fqss_amd.quantization.qat import qat_layers as QL
    form, shape, opt, mode, calls = BNFN_CASES[case]
    C = shape[1]
    cond = "1000" in case
    make = nn.BatchNorm1d if form == "1d" else nn.BatchNorm2d
    ref_bn, bn = make(C, **opt).double(), make(C, **opt)
    with torch.no_grad():
        for m in (ref_bn, bn):
            if m.affine:
                m.weight.copy_(1 + 0.3 * rnd(C, seed=1))
                m.bias.copy_(0.3 * rnd(C, seed=2))
            if m.track_running_stats:
                m.running_mean.copy_(0.2 * rnd(C, seed=3) + (700.0 if cond else 0.0))
                m.running_var.copy_(0.5 + rnd(C, seed=4).abs())
    bn32 = make(C, **opt)
    bn32.load_state_dict(bn.state_dict())
    layer = QL.BatchNormQ(bn, gradient_based=True, act_quant=False).to(DEV)
    for m in (ref_bn, bn32, layer):
        m.train(mode == "train")
    fails = []
    for call in range(calls):
        tag = f"{case}, call {call + 1}"
        x = (rnd(*shape, seed=900 + call) + (1000.0 if cond else 0.3)) * 0.7
        g = rnd(*shape, seed=950 + call)
        outs = []
        for m, xin in ((ref_bn, x.double()), (bn32, x.clone()), (layer, x.to(DEV))):
            m.zero_grad()
            xin = xin.requires_grad_(True)
            y = m(xin)
            y.backward(g.to(xin.dtype).to(xin.device))
            inner = m.batchnorm if m is layer else m
            o = {"y": y.detach(), "gx": xin.grad}
            if inner.affine:
                o.update(gw=inner.weight.grad, gb=inner.bias.grad)
            if inner.track_running_stats:
                o.update(rm=inner.running_mean.detach().clone(), rv=inner.running_var.detach().clone())
                o["nbt"] = int(inner.num_batches_tracked)
            outs.append(o)
        ref, ref32, got = outs
        assert got["y"].shape == tuple(shape) and got["gx"].shape == tuple(shape)
        if "nbt" in ref:
            assert got["nbt"] == ref["nbt"] == (call + 1 if mode == "train" else 0)
        for n in ref:
            if n != "nbt":
                measure("bnfn", n, got[n], ref[n], ref32[n], tag, fails, cond=cond and n in ("y", "gx", "gw"))
    assert not fails, fails


# ============================================================================================== per-sample normalisation, LayerScale
def sample_ref(x, biased=False):
    xd = x.double()
    return xd.mean(1), xd.std(1, unbiased=not biased)


# id -> (B, n, |mean| / std, constant input)
SAMPLE_CASES = {
    "n 2": (3, 2, 0.3, False),
    "n 50": (3, 50, 0.3, False),
    "n 262144 + 300: the moment grid (cap 256 blocks of 1024) wraps": (2, 262144 + 300, 0.3, False),
    "n 3000, mean / std 1000": (3, 3000, 1000.0, False),
    "n 3000, constant input": (2, 3000, 0.0, True),
}


@gpu
@pytest.mark.parametrize("case", list(SAMPLE_CASES))
def test_sample_norm_against_fp64(case):
    """fqss_sample_meanstd (fp64 moments; unbiased std) and fqss_sample_norm in both directions and as a round trip"""
    B, n, offset, const = SAMPLE_CASES[case]
    if "wraps" in case:
        assert -(-n // 1024) > 256
    cond = offset > 1.0
    x = torch.full((B, n), 0.7) if const else (rnd(B, n, seed=n) + offset) * 0.7
    xb, ws, ms = Vec(B * n, x), Vec(2 * B, 0.0, F64), Vec(2 * B)
    yb, zb = Vec(B * n), Vec(B * n)
    st = stream()
    _lib.call("fqss_sample_meanstd", xb.ptr, ws.ptr, ms.ptr, B, n, st)
    _lib.call("fqss_sample_norm", xb.ptr, ms.ptr, yb.ptr, B, n, 0, st)
    _lib.call("fqss_sample_norm", yb.ptr, ms.ptr, zb.ptr, B, n, 1, st)
    torch.cuda.synchronize()
    assert ms.written() and ws.guards() and yb.written() and zb.written() and xb.unchanged()
    got_ms = ms.cpu(B, 2)
    if const:
        print(f"MEAS sample constant input: std {float(got_ms[:, 1].max()):.2e}, max |y| {float(yb.t.abs().max()):.2e}")
        assert bool((got_ms[:, 0] == np.float32(0.7)).all()) and float(got_ms[:, 1].max()) <= 0.7 * 2e-7
        assert float(yb.t.abs().max()) == 0.0 and bool((zb.t == np.float32(0.7)).all())
        return
    mean, std = sample_ref(x)
    m32, s32 = x.mean(1), x.std(1)
    xd = x.double()
    fails = []
    # the mean against float64 per unit of std; its fp32 rounding is the bound
    me = float(((got_ms[:, 0].double() - mean) / std).abs().max())
    mb = (float((mean.abs() / std).max()) + 1.0) * MEAN_ULP
    print(f"MEAS sample mean |d mean| / std {me:.2e} bound {mb:.2e} | {case}")
    if not me <= mb:
        fails.append((case, "mean", me, mb))
    measure("sample", "std", got_ms[:, 1], std, s32, case, fails)
    # the fp64 moments themselves (ws: sum, sum of squares per sample), offset 1000 included
    measure("sample", "moments", ws.cpu(B, 2), torch.stack([xd.sum(1), (xd * xd).sum(1)], 1), torch.stack([x.sum(1), (x * x).sum(1)], 1), case, fails)
    ref_y = (xd - mean[:, None]) / (1e-5 + std[:, None])
    y32 = (x - m32[:, None]) / (1e-5 + s32[:, None])
    by = measure("sample", "norm", yb.cpu(B, n), ref_y, y32, case, fails, cond=cond)
    # the inverse direction on its own input (the kernel's normalised y and its fp32 statistics): y std + mean
    ref_z = yb.cpu(B, n).double() * got_ms[:, 1:2].double() + got_ms[:, 0:1].double()
    z32 = yb.cpu(B, n) * got_ms[:, 1:2] + got_ms[:, 0:1]
    measure("sample", "inv", zb.cpu(B, n), ref_z, z32, case, fails)
    # round trip: back to x up to the 1e-5 of the forward's denominator and the roundings of both passes
    trip = xd - (xd - mean[:, None]) * (1e-5 / (1e-5 + std[:, None]))
    measure("sample", "trip", zb.cpu(B, n), trip, (y32 * s32[:, None] + m32[:, None]), case, fails, cond=cond)
    assert not fails, fails
    if n == 50:
        floor("sample", "std", sample_ref(x, biased=True)[1], std, "biased instead of unbiased std", case)
    floor("sample", "norm", (xd - mean.bfloat16().double()[:, None]) / (1e-5 + std[:, None]), ref_y, "mean rounded to bf16", case, by)


@gpu
def test_chan_op_against_fp64():
    """fqss_chan_op, both modes (x * s[c], x + s[c]) on padded NaN rows, the row grid capped at 16384 included"""
    fails = []
    for B, C, M in ((3, 5, 130), (2, 9000, 3), (1, 1, 1)):
        x, s = rnd(B, C, M, seed=C), 1 + 0.3 * rnd(C, seed=C + 1)
        xb, sb = Blk(B * C, M, M + 3, 1, fill=x), Vec(C, s)
        for mode in (0, 1):
            yb = Blk(B * C, M, M + 2)
            _lib.call("fqss_chan_op", xb.ptr, sb.ptr, yb.ptr, B, C, M, xb.ld, yb.ld, mode, stream())
            torch.cuda.synchronize()
            assert yb.written()
            all_unchanged(x=xb, s=sb)
            ref = x.double() * s.double()[None, :, None] if mode == 0 else x.double() + s.double()[None, :, None]
            ref32 = x * s[None, :, None] if mode == 0 else x + s[None, :, None]
            measure("chan", "y", yb.cpu(B, C, M), ref, ref32, f"chan_op mode {mode} ({B},{C},{M})", fails)
    assert not fails, fails


# id -> (B, C, M): gxb = min(256, cdiv(M, 1024)) column blocks of 1024 (four clamped loads of stride 256 per thread), gzb =
# clamp(2048 / (gxb C), 1, B) sample slices per channel
CHAN_BWD_CASES = {
    "(7,5,1030): 2 column blocks, z split 7, clamped loads": (7, 5, 1030),
    "(7,5,1025): 2 column blocks, z split 7, one live column in the last block": (7, 5, 1025),
    "(3,3000,10): gzb 1 with a row loop": (3, 3000, 10),
}


@gpu
@pytest.mark.parametrize("case", list(CHAN_BWD_CASES))
def test_chan_scale_bwd_against_fp64(case):
    """fqss_chan_scale_bwd: gx = g s[c] and gs[c] += sum g x (fp32 sums, one atomic per workgroup; gs non-zero on entry)"""
    B, C, M = CHAN_BWD_CASES[case]
    gxb = min(256, -(-M // 1024))
    gzb = max(1, min(2048 // (gxb * C), B))
    assert ("z split 7" in case) == (gzb == 7) and ("gzb 1" in case) == (gzb == 1)
    g, x, s = rnd(B, C, M, seed=M), rnd(B, C, M, seed=M + 1), 1 + 0.3 * rnd(C, seed=2)
    gb, xb, sb = Blk(B * C, M, M + 3, fill=g), Blk(B * C, M, M + 1, 1, fill=x), Vec(C, s)
    ref_gs = (g.double() * x.double()).sum((0, 2))
    start = rnd(C, seed=3, scale=rms(ref_gs))
    ob, gsb = Blk(B * C, M, M + 2), Vec(C, start)
    _lib.call("fqss_chan_scale_bwd", gb.ptr, xb.ptr, sb.ptr, ob.ptr, gsb.ptr, B, C, M, gb.ld, xb.ld, ob.ld, stream())
    torch.cuda.synchronize()
    assert ob.written() and gsb.written()
    all_unchanged(g=gb, x=xb, s=sb)
    fails = []
    measure("chan", "gx", ob.cpu(B, C, M), g.double() * s.double()[None, :, None], g * s[None, :, None], case, fails)
    measure("chan", "gs", gsb.cpu().double() - start.double(), ref_gs, (g * x).sum((0, 2)), case, fails)
    assert not fails, fails
    floor("chan", "gs", (g.double() * x.double())[:-1].sum((0, 2)), ref_gs, "last sample dropped", case)


# id -> (R, C): rows per workgroup of k_col_scale_bwd = cdiv(R, 1024) if that is >= 32, else 32 for R >= 8192, else 8
COL_CASES = {
    "(13,24): bands of 8 rows": (13, 24, 8),
    "(8200,5): bands of 32 rows": (8200, 5, 32),
    "(32800,3): bands of cdiv(R, 1024) = 33 rows": (32800, 3, 33),
    "(9,300): C > 256, column loop": (9, 300, 8),
}


@gpu
@pytest.mark.parametrize("case", list(COL_CASES))
def test_col_scale_against_fp64(case):
    """fqss_col_scale_fwd / fqss_col_scale_bwd on channel-last rows [R][C] with padded strides; gs non-zero on entry"""
    R, C, rpb = COL_CASES[case]
    assert rpb == (-(-R // 1024) if -(-R // 1024) >= 32 else (32 if R >= 8192 else 8))
    g, x, s = rnd(R, C, seed=R), rnd(R, C, seed=R + 1), 1 + 0.3 * rnd(C, seed=2)
    gb, xb, sb = Blk(R, C, C + 3, fill=g), Blk(R, C, C + 1, 1, fill=x), Vec(C, s)
    ref_gs = (g.double() * x.double()).sum(0)
    start = rnd(C, seed=3, scale=rms(ref_gs))
    yb, ob, gsb = Blk(R, C, C + 2), Blk(R, C, C + 5), Vec(C, start)
    _lib.call("fqss_col_scale_fwd", xb.ptr, sb.ptr, yb.ptr, R, C, xb.ld, yb.ld, stream())
    _lib.call("fqss_col_scale_bwd", gb.ptr, xb.ptr, sb.ptr, ob.ptr, gsb.ptr, R, C, gb.ld, xb.ld, ob.ld, stream())
    torch.cuda.synchronize()
    assert yb.written() and ob.written() and gsb.written()
    all_unchanged(g=gb, x=xb, s=sb)
    fails = []
    measure("col", "y", yb.cpu(R, C), x.double() * s.double()[None], x * s[None], case + " fwd", fails)
    measure("col", "gx", ob.cpu(R, C), g.double() * s.double()[None], g * s[None], case, fails)
    measure("col", "gs", gsb.cpu().double() - start.double(), ref_gs, (g * x).sum(0), case, fails)
    assert not fails, fails
    floor("col", "gs", (g.double() * x.double())[:-(R % rpb or rpb)].sum(0), ref_gs, "last row band dropped", case)


# ================================================================================================================== fqss_hd_kd_loss
def hd_ref(est, fest, src, wt, lam, dtype=F64, no_eps=False, sgn0_plus=False):
    """the HTDemucs training loss of csrc/hd_loss.hip's header in `dtype`: est / fest / src [B, S, N], wt [S] -> loss, task [S], kd [S],
    w [B, S], grad [B, S, N] = ct sign(est - src) + ck sign(est - fest).  no_eps: new_sdr without its 1e-7 terms; sgn0_plus: sign(0) = +1"""
    e, f, s, wt = (t.to(dtype) for t in (est, fest, src, wt))
    B, S, N = e.shape
    lam = float(np.float32(lam))
    eps = 0.0 if no_eps else 1e-7
    d1, d2 = e - s, e - f
    num = (s * s).sum(-1) + eps
    sdr_t = 10.0 * torch.log10(num / (((s - f) ** 2).sum(-1) + eps))
    sdr_q = 10.0 * torch.log10(num / (((s - e) ** 2).sum(-1) + eps))
    w = torch.exp((sdr_t - sdr_q) / 10.0)
    task = d1.abs().mean(-1).mean(0)
    kd = (w * d2.abs().mean(-1)).mean(0)
    loss = (wt * ((1.0 - lam) * task + lam * kd)).sum() / wt.sum()
    ct = wt / wt.sum() * (1.0 - lam) / (B * N)
    ck = (wt / wt.sum())[None, :] * lam * w / (B * N)
    sg = (lambda d: torch.where(d >= 0, 1.0, -1.0).to(dtype)) if sgn0_plus else torch.sign
    return {"loss": loss.reshape(1), "task": task, "kd": kd, "w": w, "grad": ct[None, :, None] * sg(d1) + ck[..., None] * sg(d2)}


def hd_operands(B, S, N, seed):
    """est / fest near src (0.1 / 0.05 off).  From S = 4 on: source 1 silent (src = 0, the teacher 1e-4 off it, so that the 1e-7 of
    new_sdr's denominator carries 0.3 % of it); (b 0, s 2): est == fest exactly; (b B-1, s 3): est == src on [100, 400)"""
    src = rnd(B, S, N, seed=seed)
    est, fest = src + 0.1 * rnd(B, S, N, seed=seed + 1), src + 0.05 * rnd(B, S, N, seed=seed + 2)
    if S >= 4:
        src[:, 1] = 0.0
        fest[:, 1] = 1e-4 * rnd(B, N, seed=seed + 3)
        est[:, 1] = 0.1 * rnd(B, N, seed=seed + 4)
        fest[0, 2] = est[0, 2]
        est[B - 1, 3, 100:400] = src[B - 1, 3, 100:400]
    return est, fest, src


# id -> (B, S, N), source weights, kd_lambda
HD_CASES = {
    "(2,4,3000) lambda 0.1": ((2, 4, 3000), [0.0, 1.0, 0.5, 2.5], 0.1),
    "(2,4,3000) lambda 0": ((2, 4, 3000), [0.0, 1.0, 0.5, 2.5], 0.0),
    "(2,4,3000) lambda 1": ((2, 4, 3000), [0.0, 1.0, 0.5, 2.5], 1.0),
    "(1,1,1)": ((1, 1, 1), [0.7], 0.1),
    "(1,2,524288 + 300): the grid (256 blocks of 2048) wraps": ((1, 2, 524288 + 300), [1.0, 2.0], 0.1),
}


def hd_run(est, fest, src, wt, lam, want_grad=True):
    B, S, N = est.shape
    eb, fb, sb, wb = Vec(B * S * N, est), Vec(B * S * N, fest), Vec(B * S * N, src), Vec(S, wt)
    sums, out, coef = Vec(5 * B * S, 0.0, F64), Vec(1 + 2 * S + B * S), Vec(2 * B * S)
    gb = Vec(B * S * N) if want_grad else None
    _lib.call("fqss_hd_kd_loss", eb.ptr, fb.ptr, sb.ptr, wb.ptr, sums.ptr, out.ptr, coef.ptr, gb.ptr if want_grad else None, B, S, N, float(lam),
              stream())
    torch.cuda.synchronize()
    assert out.written() and coef.written() and sums.written() and (gb is None or gb.written())
    all_unchanged(est=eb, fest=fb, src=sb, wt=wb)
    o = out.cpu()
    got = {"loss": o[:1], "task": o[1:1 + S], "kd": o[1 + S:1 + 2 * S], "w": o[1 + 2 * S:].reshape(B, S)}
    if want_grad:
        got["grad"] = gb.cpu(B, S, N)
    return got


@gpu
@pytest.mark.parametrize("case", list(HD_CASES))
def test_hd_kd_loss_against_fp64(case):
    """fqss_hd_kd_loss: loss, task_s, kd_s, w and d loss / d est against float64, with a silent source, est == fest on one (b, s), est == src
    on a block (the gradient's task term is exactly 0 there), a zero source weight; want_grad = False gives the same numbers"""
    (B, S, N), wt, lam = HD_CASES[case]
    if "wraps" in case:
        assert N > 256 * 2048
    ops = hd_operands(B, S, N, seed=N % 1000 + S)
    wt = torch.tensor(wt)
    ref, ref32 = hd_ref(*ops, wt, lam), hd_ref(*ops, wt, lam, dtype=torch.float32)
    got = hd_run(*ops, wt, lam)
    nograd = hd_run(*ops, wt, lam, want_grad=False)
    fails = []
    for n in ("loss", "task", "kd", "w"):
        assert bool(torch.equal(got[n], nograd[n])), f"{n}: want_grad = False changes it"
        measure("loss", n, got[n], ref[n], ref32[n], case, fails)
    if float(ref["grad"].abs().max()) > 0:
        measure("loss", "grad", got["grad"], ref["grad"], ref32["grad"], case, fails)
    assert not fails, fails
    if S >= 4:
        e, f, s = ops
        g = got["grad"].double()
        assert bool((g[:, 0] == 0).all()), "a zero source weight must give a zero gradient"
        if lam == 1.0:
            assert bool((g[0, 2] == 0).all()), "est == fest and no task term: the gradient is exactly 0"
        assert float(got["w"][0, 2]) == 1.0, "est == fest: both SDRs are the same number"
        blk = g[B - 1, 3, 100:400]
        ck = float(ref["grad"][B - 1, 3, 100:400].abs().max())
        assert float(blk.abs().max()) <= ck * (1 + 1e-5), "est == src: only the distillation term is left on the block"
        floor("loss", "grad", hd_ref(*ops, wt, lam, sgn0_plus=True)["grad"], ref["grad"], "sgn(0) taken as +1", case)
        if lam == 0.1:
            floor("loss", "w", hd_ref(*ops, wt, lam, no_eps=True)["w"], ref["w"], "1e-7 omitted on the silent source", case)


@gpu
def test_hd_kd_loss_row_limit():
    """B S = 65535 with N = 1 runs and meets the bounds; B S = 65536 is refused with nothing written"""
    B, S, N = 13107, 5, 1
    assert B * S == 65535
    ops = hd_operands(B, S, N, seed=5)
    wt = torch.tensor([1.0, 0.5, 2.0, 0.0, 1.5])
    ref, ref32 = hd_ref(*ops, wt, 0.1), hd_ref(*ops, wt, 0.1, dtype=torch.float32)
    got = hd_run(*ops, wt, 0.1)
    fails = []
    # (N = 1: every w is exp of the difference of two single-sample SDRs, tens of dB apart, through log10f / expf: the gradient takes
    # COND x torch fp32's own error on this case, the three sums the bounds of the ordinary cases)
    for n in ("loss", "task", "kd", "grad"):
        measure("loss", n, got[n], ref[n], ref32[n], "B S = 65535, N = 1", fails, cond=n == "grad")
    assert not fails, fails
    B = 16384
    eb, wb = Vec(B * 4, rnd(B * 4)), Vec(4, 1.0)
    sums, out, coef, gb = Vec(5 * B * 4, 0.0, F64), Vec(1 + 8 + B * 4), Vec(2 * B * 4), Vec(B * 4)
    refused("fqss_hd_kd_loss", eb.ptr, eb.ptr, eb.ptr, wb.ptr, sums.ptr, out.ptr, coef.ptr, gb.ptr, B, 4, 1, 0.1, stream())
    assert out.untouched() and coef.untouched() and gb.untouched() and sums.unchanged()


# =============================================================================================================== deterministic mode
@pytest.fixture
def det_off():
    yield
    if K is not None:
        K.DetMode.off()          # (the control block is device-wide: no later test may run under it)


@gpu
def test_deterministic_gradient_sums_against_fp64(det_off):
    """FQSS_DETERMINISTIC=1 arithmetic (fqss_dev.h grad_add: integer sums on the shadow of the attached slot-0 arena, fqss_det_finish
    rounds once) for the three fp32 gradient atomics of this family -- k_dwconv_bwd_w, k_chan_scale_bwd and the nbs > 1 branch of
    k_gn_bwd_coef -- into slices of that arena: two runs are bit-identical and both meet the float64 bounds of the atomic path"""
    # depthwise weight gradient
    B, C, M, Kt, dil, pad = 3, 7, 131, 5, 3, 6
    x, gz, w = rnd(B, C, M, seed=1), rnd(B, C, M, seed=2), rnd(C, Kt, seed=3)
    dref = dw_ref(x, w, None, gz, dil, pad)
    xb, gzb = Blk(B * C, M, pad4(M), fill=x), Blk(B * C, M, pad4(M), fill=gz)
    # LayerScale gradient
    B2, C2, M2 = 7, 5, 1030
    g2, x2, s2 = rnd(B2, C2, M2, seed=4), rnd(B2, C2, M2, seed=5), 1 + 0.3 * rnd(C2, seed=6)
    g2b, x2b, s2b, o2b = Blk(B2 * C2, M2, fill=g2), Blk(B2 * C2, M2, fill=x2), Vec(C2, s2), Blk(B2 * C2, M2)
    ref_gs = (g2.double() * x2.double()).sum((0, 2))
    # GroupNorm parameter gradients, B = 17: nbs = 2
    B3, C3, M3 = 17, 6, 21
    assert gn_nbs(B3) == 2
    ops3 = gn_operands(B3, C3, M3, seed=7)
    gref = gn_ref(*ops3, GN_EPS)
    run3 = GnRun(ops3, gn_layout(M3, "pad")).forward()
    arena = torch.zeros(256, device=DEV)
    slot = {"gw": arena[0:C * Kt], "gs": arena[64:64 + C2], "gg": arena[128:128 + C3], "gb": arena[192:192 + C3]}
    start = {"gw": rnd(C * Kt, seed=8, scale=rms(dref["gw"])), "gs": rnd(C2, seed=9, scale=rms(ref_gs)),
             "gg": rnd(C3, seed=10, scale=rms(gref["ggamma"])), "gb": rnd(C3, seed=11, scale=rms(gref["gbeta"]))}
    det = K.DetMode()
    det.attach(0, arena)
    det.activate()
    runs = []
    for _ in range(2):
        arena.zero_()
        for n, sl in slot.items():
            sl.copy_(start[n])
        _lib.call("fqss_dwconv_bwd_w", gzb.ptr, xb.ptr, slot["gw"].data_ptr(), B, C, M, Kt, dil, pad, gzb.ld, xb.ld, stream())
        _lib.call("fqss_chan_scale_bwd", g2b.ptr, x2b.ptr, s2b.ptr, o2b.ptr, slot["gs"].data_ptr(), B2, C2, M2, g2b.ld, x2b.ld, o2b.ld, stream())
        run3.backward(None, slots=(slot["gg"], slot["gb"]))
        det.finish(0)
        torch.cuda.synchronize()
        runs.append(arena.cpu().clone())
    K.DetMode.off()
    assert bool(torch.equal(runs[0], runs[1])), "deterministic mode: the sums of two runs differ"
    a = runs[0]
    gaps = torch.ones_like(a, dtype=torch.bool)
    off = {"gw": 0, "gs": 64, "gg": 128, "gb": 192}
    for n, sl in slot.items():
        gaps[off[n]:off[n] + sl.numel()] = False
    assert bool((a[gaps] == 0).all()), "a write between the gradient slots"
    add = {n: a[off[n]:off[n] + sl.numel()].double() - start[n].double() for n, sl in slot.items()}
    fails = []
    measure("dw", "gw", add["gw"].reshape(C, Kt), dref["gw"], None, "deterministic k_dwconv_bwd_w", fails)
    measure("chan", "gs", add["gs"], ref_gs, None, "deterministic k_chan_scale_bwd", fails)
    measure("gn", "ggamma", add["gg"], gref["ggamma"], None, "deterministic k_gn_bwd_coef nbs 2", fails)
    measure("gn", "gbeta", add["gb"], gref["gbeta"], None, "deterministic k_gn_bwd_coef nbs 2", fails)
    measure("gn", "gx", run3.gx.cpu(B3, C3, M3), gref["gx"], None, "deterministic mode, gx", fails)
    assert not fails, fails


# ==================================================================================================== the references, without a GPU
def test_references_on_cpu():
    """The closed forms this file measures the kernels against, checked in float64 against torch's own group_norm / batch_norm / conv1d
    autograd and oracle.fqss_oracle (act_quantize, act_indices): the quantized GroupNorm with its STE and range gradients, the loss of
    fqss_hd_kd_loss with its gradient, and the launch-path arithmetic restated from the kernels' launch code.  Needs no device."""
    tight = lambda a, b: float((a.double() - b.double()).abs().max()) <= 1e-11 * max(1.0, float(b.double().abs().max()))     # noqa: E731
    for (B, C, M), q in (((2, 3, 50), None), ((3, 4, 33), QRANGE), ((17, 6, 21), QRANGE)):
        ops = gn_operands(B, C, M, seed=B + M)
        ref, tor = gn_ref(*ops, GN_EPS, q=q), gn_torch(*ops, GN_EPS, F64, q=q)
        for n in ("y", "pre", "mean", "rstd", "gx", "ggamma", "gbeta") + (("glo", "ghi") if q else ()):
            assert tight(ref[n], tor[n]), (n, q)
        if q:
            assert bool(torch.equal(ref["codes"], tor["codes"]))
            assert 0.01 <= 1.0 - float(ref["inr"].double().mean()) <= 0.08
        # and as batch_norm over the one "channel" a sample is: group_norm(1, C) = batch_norm of [1, B, C M] without affine
        x = ops[0].double()
        bnv = F.batch_norm(x.reshape(1, B, C * M), None, None, training=True, eps=GN_EPS).reshape(B, C, M)
        assert tight(gn_ref(ops[0], ops[1], torch.ones(C), torch.zeros(C), GN_EPS)["pre"], bnv)
    # the mutations are what they say
    x = gn_operands(2, 3, 8200, seed=1)[0]
    m0, v0 = gn_moments(x)
    m1, v1 = gn_moments(x, drop_slice=(4, 3))
    kept = torch.cat([x[..., c0:c0 + 1024] for c0 in range(0, 8200, 1024) if (c0 // 1024) % 3 != 2], -1).double()
    assert tight(m1, kept.sum((1, 2)) / (3 * 8200)) and float((m1 - m0).abs().min()) > 0.05
    # the loss: gradient by autograd of the same scalar (w detached), sign(0) = 0 on est == src / est == fest
    est, fest, src = hd_operands(2, 4, 300, seed=3)
    est[1, 3, 100:200] = src[1, 3, 100:200]
    wt = torch.tensor([0.0, 1.0, 0.5, 2.5])
    for lam in (0.0, 0.1, 1.0):
        ref = hd_ref(est, fest, src, wt, lam)
        e = est.double().requires_grad_(True)
        lam32 = float(np.float32(lam))
        f, s = fest.double(), src.double()
        sdr = lambda xx: 10 * torch.log10(((s * s).sum(-1) + 1e-7) / (((s - xx) ** 2).sum(-1) + 1e-7))     # noqa: E731
        w = torch.exp((sdr(f) - sdr(e)) / 10).detach()
        task = torch.stack([F.l1_loss(e[:, i], s[:, i]) for i in range(4)])
        kd = torch.stack([(w[:, i, None] * (e[:, i] - f[:, i]).abs()).mean() for i in range(4)])
        loss = (wt.double() * ((1 - lam32) * task + lam32 * kd)).sum() / wt.sum()
        loss.backward()
        assert tight(ref["loss"], loss.detach().reshape(1)) and tight(ref["task"], task.detach()) and tight(ref["kd"], kd.detach())
        assert tight(ref["w"], w) and float((ref["grad"] - e.grad).abs().max()) <= 1e-15
        assert bool((ref["grad"][:, 0] == 0).all())
    assert float(hd_ref(est, fest, src, wt, 0.1, sgn0_plus=True)["grad"][1, 3, 100:200].abs().min()) > 0
    # the depthwise reference against an explicit tap loop
    x, w, gz = rnd(2, 3, 40, seed=1), rnd(3, 5, seed=2), rnd(2, 3, 40, seed=3)
    ref = dw_ref(x, w, None, gz, 3, 6)
    z = torch.zeros(2, 3, 40, dtype=F64)
    for k in range(5):
        for m in range(40):
            src_m = m + 3 * k - 6
            if 0 <= src_m < 40:
                z[:, :, m] += w.double()[:, k] * x.double()[:, :, src_m]
    assert tight(ref["z"], z)
    # launch-path arithmetic quoted by the issue
    assert gn_slices(6, 8200, 4) == 3 and gn_slices(5, 4099, 1) == 5 and gn_slices(6, 4096, 4) == 1 and gn_slices(512, 10 ** 6, 4) == 1
    assert (gn_nbs(16), gn_nbs(17), gn_nbs(40), gn_nbs(5000)) == (1, 2, 3, 64)
    assert (bn_grid(5, 1), bn_grid(3, 700), bn_grid(2, 1100), bn_grid(300, 3)) == (5, 2, 1, 300)
