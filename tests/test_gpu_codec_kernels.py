"""The waveform codec kernels -- csrc/codec.hip: the 8-bit splitter (k_splitter2, k_row_absmax + k_splitter2_rows, k_splitter2_raw), the
framing convolution (k_frames_conv4 / k_frames_conv_fwd), the transposed convolution with overlap-add (k_ola_mfma16 / k_ola_convtr_fwd, three
operand modes) and the Ci = 1 weight gradient on the fp32 matrix cores (k_frames_wgrad_mfma, fp32 and coded), with its fallback
fqss_frames_wgrad of csrc/gemm.hip (launch_gemm with a strided B operand) -- at the C ABI, against exact integers and float64.  The entry
points are called through fqss_amd._lib with explicit pointers and leading dimensions, in the manner of tests/test_gpu_qgemm_kernels.py and
tests/test_gpu_rowgemm_kernels.py, whose buffers and helpers this file imports.  The case bodies take the backend from the module
(tests/test_codec_cpu.py runs them on libfqss_cpu.so for the entries that library has).

Entry points covered: fqss_splitter2, fqss_splitter2_rows, fqss_splitter2_raw; fqss_frames_conv_fwd, fqss_frames_conv_add_fwd;
fqss_ola_convtr_fwd, fqss_ola_convtr_fwd_q, fqss_ola_convtr_mul_fwd; fqss_frames_wgrad, fqss_frames_wgrad1, fqss_frames_wgrad1s,
fqss_frames_wgrad1_q; and the deterministic-mode form of the weight gradients' atomics.  Every entry has guarded-buffer cases and one
refusal per FQSS_REQUIRE / set_error the flat ABI can reach (test_*_refusals).  Not reachable there: the `if (NS < 1) NS = 1` of
ola_convtr_impl (the masking REQUIRE in front refuses NS < 1, the other modes pass 1); "unsupported operand layout" of launch_gemm under
fqss_frames_wgrad (the entry passes the layout itself); T < 1 of frames_wgrad1_launch (the "frames exceed the signal" REQUIRE in front
needs T >= K).  N > 65535 is refused by the conv, the decoder and the _wgrad1 trio; fqss_frames_wgrad has no such REQUIRE (its batch is
grid.z of launch_gemm) and is not called with one here.

Layout under test.  fp32 operands sit in NaN-filled flat buffers between guard floats, row padding stays NaN; code operands sit in
0xA5-filled buffers between guard bytes; outputs are NaN-filled, gw starts from non-zero random values (it accumulates).  The operands of a
case have different ld's and at least one has padding beyond what its alignment rule asks for.  After each call: every operand
bit-identical, the guards untouched, every live output element finite and nothing outside the permitted region written.  The permitted
region (include/fqss.h states it since this file): k_frames_conv4 columns [0, (M + 3) & ~3) of a z row (whole float4 stores; what lands in
[M, (M + 3) & ~3) is unspecified and may be NaN), the generic framing conv [0, M); both decoder forms exactly [0, T) of every out row;
the weight gradients exactly C x K (row stride ld_gw for fqss_frames_wgrad1s, the other column blocks of a row bit-identical).

Dispatch.  No library switch: the same live values go into an aligned and a deliberately disqualified buffer.
  framing conv   k_frames_conv4 iff (K, S) in {(16, 8), (32, 16)}, Ci in {1, 2}, x 16-B aligned, T % 4 == 0, z (and add) 16-B aligned with
                 ld % 4 == 0 and ld >= roundup4(M); else k_frames_conv_fwd.  Disqualifiers used: "xoff" x one float off, "todd" T % 4 != 0
                 (tail samples no frame covers), "ldodd" ld_z % 4 == 1, "zoff" z one float off, "short" ld_z = M < roundup4(M),
                 "addoff" / "addodd" the addend.  Both forms run the same j-ordered fmaf chain: torch.equal.
  decoder        k_ola_mfma16 iff (K, S) = (16, 8), operand rows 16-B aligned with ld >= roundup4(M) and ld % 4 == 0 (codes: ld % 16 == 0;
                 masking form: feat alike); else k_ola_convtr_fwd.  Disqualifiers: "odd" ld % 4 == 1 (codes: ld % 16 == 4), "off" base one
                 float (byte) off.  The forms sum the channels in different orders (a contiguous block per wave in MFMA steps of four
                 against every fourth channel per wave): each against float64, the pair within the sum of the bounds, bit-equal on integers.
  wgrad          k_frames_wgrad_mfma iff (K, S) in {(16, 8), (32, 16)} and 16-B rows (fp32 ld_a % 4, codes ld_a % 16), else FQSS_EINVAL;
                 fqss_frames_wgrad is launch_gemm on any layout.
Named shapes and the dispatch values they produce (conv_dispatch / wgrad1_dispatch mirror the launch code; test_codec_cpu.py and
test_dispatch_of_the_named_shapes assert them, so a change of the heuristics fails here instead of un-testing a path):
  framing conv (N, Ci, Co, M, K, S)        zs  co_per  co_tile  tiles per slice   last slice
    (2, 2, 24, 77, 16, 8)                   1    24      24          1               24       the baseline
    (2, 1, 100, 300, 16, 8)                 3    36      36          1               28       ragged last slice (28 = 3 prefetch groups + 4)
    (1, 2, 70, 257, 16, 8)                  2    36      36          1               34       M just past one workgroup's 256 frames
    (512, 2, 200, 8, 32, 16)                1   200     192          2 (192 + 8)    200       second LDS tap tile
    (512, 2, 197, 5, 32, 16)                1   200     192          2 (192 + 5)    197       ... with Co % 4 != 0
    (600, 1, 770, 3, 16, 8)                 1   772     768          2 (768 + 2)    770       second tile at Ci = 1
  wgrad (N, C, M)            fp32: msplit  mchunk  passes  last chunk     coded: msplit  mchunk  passes  last chunk
    (512, 8, 300)                    1      384      3       300                   1      512      2       300
    (1, 8, 2100)                     9      256      2        52                   9      256      1        52
    (1, 8, 4200)                    11      384      3       360                   9      512      2       104
    (3, 130, 513)                    5      128      1         1                   3      256      1         1

Exact-integer cases (torch.equal, no tolerance) for every form of the conv, the decoder and the weight gradients: small integer operands,
coded operands with the range [lo, lo + 255] (delta = 1), limits chosen per case so that the sum of the absolute values of every term
(the start of gw included) stays below 2^24 -- asserted on the CPU per case (exact_ok) -- so fp32 is exact in every order: these cases hold
the atomics, the LDS cross-wave sums and the split partial sums to "every term exactly once".

Against float64 with real operands (a DC offset on the waveforms: they are not zero-mean at chunk scale).
  framing conv: the bound is derived, not measured.  One fmaf chain of n = Ci K terms from 0 (n roundings), one more for the addend:
     |z - ref| <= (n + 2) 2^-24 (sum_j |x_j w_j| + |add|)    per element (gamma_n = n u / (1 - n u), n <= 64: the + 2 covers the addend's
  rounding and the second-order terms).
  decoder / weight gradients: measured on the MI355X, largest e_elem / e_norm over a family's cases beside torch fp32 on the CPU on the
  same cases; BOUND below is at most 4 x the measurement:
                                        kernel               fp32                 bound                 worst case
    k_ola_mfma16       (three modes)  out   4.82e-7 / 9.10e-8    1.42e-6 / 2.47e-7    1.5e-6 / 3.2e-7    3.1 / 3.5   (3, 33, 119) mode 2; (1, 4, 3) mode 1
    k_ola_convtr_fwd   (three modes)  out   6.42e-7 / 1.07e-7    1.42e-6 / 2.50e-7    1.8e-6 / 3.7e-7    2.8 / 3.5   (1, 5, 62, 32, 16) mode 2; (1, 4, 3) mode 1
    k_frames_wgrad_mfma fp32 (_wgrad1, _wgrad1s)  gw   3.42e-6 / 7.61e-7    2.32e-6 / 5.59e-7    1.2e-5 / 2.6e-6    3.5 / 3.4   (512, 8, 300) _wgrad1s; deterministic
                                                                                                                    mode 5.9e-7 / 1.9e-7
    k_frames_wgrad_mfma coded (_wgrad1_q)         gw   2.33e-6 / 6.98e-7    1.18e-6 / 4.21e-7    8.1e-6 / 2.4e-6    3.5 / 3.4   (512, 8, 300); deterministic 3.3e-7 / 6.2e-8
    fqss_frames_wgrad (k_gemm_f32, both VEC)      gw   4.01e-6 / 8.11e-7    3.40e-6 / 6.13e-7    1.4e-5 / 2.8e-6    3.5 / 3.5   (512, 8, 300) Ci = 2; deterministic
                                                                                                                    mode 8.0e-7 / 1.5e-7
  (two runs: the weight gradients go through fp32 atomics and differ from run to run, the fallback by 3.1e-6 .. 4.0e-6.)  The framing
  conv reaches at most 0.44 of its derived per-element bound, torch fp32 F.conv1d 0.44 of it on the same cases.  No family sits above its
  fp32 yardstick by more than a factor 2.0 (coded wgrad; fp32 wgrad 1.5, fallback 1.3, the decoders below it: torch accumulates the
  transposed conv in another order).  fqss_frames_wgrad1 against fqss_frames_wgrad on the same operands: at most 2.7e-6; the decoder's two
  forms against each other at most 7.5e-7.
  Bit-exact, no bound: every exact-integer case; k_frames_conv4 against k_frames_conv_fwd on the live columns of every conv case, with
  and without the addend; the splitters; fqss_ola_convtr_fwd_q against fqss_decode + fqss_ola_convtr_fwd and fqss_ola_convtr_mul_fwd
  against fqss_mul_bcast_fwd + fqss_ola_convtr_fwd when both calls take the same form (both matrix-core: code rows ld % 16 == 0 / decoded
  rows ld % 4 == 0; or both generic) -- in all 16 cases, NS in {1, 2, 3}.  With the fused call in one form and the chain's decoder in the
  other ("MIXED" lines) the results are NOT bit-identical: they differ in 9 of the 10 real-valued (16, 8) cases in either direction (equal
  only at C = 1 and on integers), so the header's claim holds under that condition only, which include/fqss.h now states.
  Deterministic mode: two runs bit-equal after fqss_det_finish, the integer slots exact, nothing beside the slots.

Splitter: bit for bit (torch.equal on the bit images) against a float32 emulation on the CPU in process.py's op order --
oracle.fqss_oracle.split for the normalised form, split_raw_emul below for normalize=False (process.py:26-36), split_rows_emul = split per
row; test_codec_cpu.py ties them to the reference-generated fixture tests/golden/codec_split.npz (tools/make_goldens_codec.py).  Inputs:
multiples of thr / 128, +-thr (thr clamps to 127), +-0, denormals; for _rows, rows at levels 1, 1e-3, 7 and 1e-30 and one silent row,
which is NaN in that row only (0 / 0 through torch.clip, which propagates NaN) while the other rows are unaffected.

Mutation floors: e_elem of the wrong kernel, computed in float64 on the CPU on each case's own operands, asserted 10 x above the bound in
every non-void case (for the framing conv in units of the element's derived bound, where 10 is asked); for the exact cases the share of
elements that differ is printed and must be non-zero.
    framing conv (x the element's bound; smallest over the cases, all at (2, 2, 3, 3, 32, 16)): last frame dropped 6.1e4; last channel dropped
                 7.9e4 (void at Ci = 1); a tap row of the neighbouring channel 1.5e5 (void at Co = 1); frame index one off 6.8e4 (void at
                 M = 1); last tap dropped 5.0e3; the addend dropped 1.0e5; ld_add read as ld_z 1.6e5 (void for one row, N Co = 1).  Exact
                 cases, smallest share of elements that differ: last frame dropped 0.0033 (1 frame of 300), ld_add read as ld_z 0.67, the
                 others >= 0.91
    decoder      (both forms alike) last frame dropped 0.54; last channel dropped 6.1e-2 (C = 130; void at C = 1); one wave's channel block
                 dropped 0.51 (void at C <= 4); a tap row of the neighbouring channel 0.67 (void at C = 1); frame index one off 0.63 (void
                 at M = 1); the overlap term (r = 1) dropped 0.82 (void at M = 1); padding column M read as a value of the rms 0.62.  Exact:
                 padding column M read 0.0082 (the 8 shared samples of 976), last frame dropped 0.010, the others >= 0.33
    wgrad fp32   (_wgrad1, _wgrad1s, fallback) last frame dropped 4.1e-2 and padding column M read as a value of the rms 2.8e-2 (M = 4200, the
                 most diluted case); frame index one off 1.9 (void at M = 1); the operand row of the neighbouring channel 2.5 (void at
                 C = 1); one split chunk added twice 0.83 (void at msplit = 1); _wgrad1s: the other channel's signal 2.8
    wgrad coded  last frame dropped 3.4e-3 and padding column M read 1.0e-3 (M = 4200; the operand's mean 0.59 carries the sum, so one frame
                 of 4200 weighs less than in the zero-mean fp32 cases -- still 128 x the bound); frame index one off 1.8e-2; the operand row
                 of the neighbouring channel 2.5e-2; one split chunk added twice 0.15; min_a dropped 1.2.  Exact: >= 0.44 everywhere
    splitter     round instead of floor: 0.59 of the elements differ (normalised and raw), 0.62 (rows); the global threshold where the row
                 threshold belongs: counted on rows at levels 1, 1e-3, 7, 1e-30
  Checked once on the MI355X against scratch copies of the library carrying ONE mutation each (built outside the package, never committed;
  every access stays in bounds):
    the tail-frame mask fv[j] of k_ola_mfma16 dropped (the select that keeps NaN row padding and clamped groups out) -- 20 tests fail:
      test_decoder_exact_integers and test_decoder_against_fp64 at every (16, 8) case;
    the overlap term (r = 1) of k_ola_convtr_fwd dropped -- 32: both decoder tests at all 16 cases;
    the last of the four addend values of k_frames_conv4 replaced by the third -- 20: test_frames_conv_exact_integers / _against_fp64 at
      the ten cases whose fourth frame of a group is live;
    the channel mask c < C of k_frames_wgrad_mfma's adds replaced by a clamp (rows past C added into row C - 1) -- 27: both weight-gradient
      tests at the 13 cases with C % 64 != 0, and test_frames_wgrad_deterministic_mode;
    one frame of the neighbouring split chunk added twice (mend one too far) -- 15: both weight-gradient tests at the seven cases with more
      than one chunk, and deterministic mode;
    rintf for floorf in split_q -- 2: test_splitter_bit_for_bit, test_splitter_rows_bit_for_bit.
    Void: the frame mask of k_frames_wgrad_mfma against M instead of the chunk end passes every test -- and is the same kernel: mchunk is a
    multiple of the workgroup step, so a pass only runs past the chunk end where the chunk end is M.

Defects found and fixed with this file:
    1. The splitters returned -1.0, not NaN, for a silent row / an all-zero tensor: split_q clamped with fminf(fmaxf(v, -128), 127), which
       returns the bound for a NaN operand, where process.quantize's torch.clip propagates the NaN of 0 / 0 -- and include/fqss.h promised
       "a silent row is NaN in that row only".  Failing case: test_splitter_rows_bit_for_bit (row 4 of the level case; on the CPU backend
       tests/test_codec_cpu.py::test_splitter_on_the_cpu_backend, where the same clamp stood).  Fixed in csrc/codec.hip (split_clip, all
       three kernels) and csrc/cpu/fqss_cpu.cpp: compare-and-select, bit-identical for every non-NaN input.
    Nothing else: every other case of this file passes on the kernels of the parent commit.  That establishes that the clamped loads
    (min(idx, T - 4), min(m0, ld_a - 16), min(c, C - 1)) and the masks by select keep NaN row padding and 0xA5 code padding out of every
    result; that the second LDS tap tile, the ragged last slice and the clamped addend rows of k_frames_conv4 compute what the generic form
    computes; that the multi-pass and split frame loops of k_frames_wgrad_mfma add every term once; and that no entry writes outside the
    region the header now states.  fqss_decode stores whole float4s into its output's row padding (seen through this file's chain runs):
    documented behaviour of that entry, outside this family.

References: plain float64 torch on the CPU from the formulas in include/fqss.h; tests/test_codec_cpu.py::test_references_on_cpu ties them to
float64 F.conv1d, F.conv_transpose1d and their autograd.  e_elem = max |got - ref| / rms(ref), e_norm = ||got - ref|| / ||ref||; the
yardstick is the same operation in torch fp32 on the CPU ("MEAS" lines)."""
import pytest
import torch
import torch.nn.functional as F

import oracle.fqss_oracle as O
import tests.test_gpu_layout_spectral_kernels as L
import tests.test_gpu_qgemm_kernels as Q
from tests.test_gpu_layout_spectral_kernels import EINVAL, F64, G, NAN, Blk, Vec, all_unchanged, errs, gpu, rms  # noqa: F401
from tests.test_gpu_qgemm_kernels import (GB, SENT, TWO24, ULP, Cod, codes, delta32, differs, exact_ok, f32, fwritten, gen, heavy, ints,  # noqa: F401
                                          r4, r16, sc)

K = None
_lib = None

# per family and tensor: (e_elem bound, e_norm bound), at most 4 x the largest figure measured on the MI355X over the family's cases
BOUND = {
    "ola_mfma": {"out": (1.5e-6, 3.2e-7)},
    "ola_gen": {"out": (1.8e-6, 3.7e-7)},
    "wg1": {"gw": (1.2e-5, 2.6e-6)},
    "wg1q": {"gw": (8.1e-6, 2.4e-6)},
    "wgfb": {"gw": (1.4e-5, 2.8e-6)},
}


@pytest.fixture(scope="module")
def _gpu():
    global K, _lib
    L._gpu_fixture()
    K, _lib = L.K, L._lib
    yield


def on_gpu():
    return L.DEV == "cuda"


def sync():
    if on_gpu():
        torch.cuda.synchronize()


def stream():
    return torch.cuda.current_stream().cuda_stream if on_gpu() else None


def have(name):
    """the backend has this entry (libfqss_cpu.so serves a subset)"""
    return hasattr(_lib.load(), name)


def call(name, *args):
    _lib.call(name, *args)
    sync()


def refused(name, *args, who=None):
    """the entry returns FQSS_EINVAL and fqss_last_error names it (who: the helper that speaks for it)"""
    rc = _lib._bind(name)(*args)
    msg = _lib.load().fqss_last_error().decode()
    sync()
    assert rc == EINVAL and (who or name) in msg, (name, rc, msg)
    return msg


def measure(fam, name, got, ref, ref32, tag, fails):
    L.measure(fam, name, got, ref, ref32, tag, fails, bound=BOUND[fam][name])


def floor(fam, name, mut, ref, what, tag, fails):
    """L.floor, collected instead of raised at once (every floor of a case is printed)"""
    try:
        L.floor(fam, name, mut, ref, what, tag, bound=BOUND[fam][name])
    except AssertionError as e:
        fails.append(("floor", e.args[0]))


def cdiv(a, b):
    return -(-a // b)


def ptr(v):
    return v.ptr if v is not None else None


# =============================================================================================== the launch code, mirrored on the CPU
def conv_dispatch(N, Ci, Co, M, K_, S, T, x_al=True, z_al=True, ld_z=None, add_al=True, ld_add=None):
    """frames_conv_impl of csrc/codec.hip: the form and, for k_frames_conv4, the slicing of the output channels"""
    m4 = r4(M)
    ld_z = m4 if ld_z is None else ld_z
    ok = (K_, S) in ((16, 8), (32, 16)) and Ci in (1, 2) and x_al and T % 4 == 0 and T >= 4 and z_al and ld_z % 4 == 0 and ld_z >= m4
    if ld_add is not None:
        ok = ok and add_al and ld_add % 4 == 0 and ld_add >= m4
    if not ok:
        return dict(form="generic", grid=(cdiv(M, 64), N))
    co_tile = (48 * 1024 // (Ci * K_ * 4)) & ~3
    if co_tile > Co:
        co_tile = r4(Co)
    zs = max(1, min(cdiv(512, cdiv(M, 256) * N), Co // 32))
    co_per = cdiv(cdiv(Co, zs), 4) * 4
    zs = cdiv(Co, co_per)
    co_tile = min(co_tile, co_per)
    last = Co - (zs - 1) * co_per
    return dict(form="conv4", zs=zs, co_per=co_per, co_tile=co_tile, tiles=cdiv(min(co_per, Co), co_tile), last=last,
                grid=(cdiv(M, 256), N, zs))


def ola_dispatch(mode, C, M, K_, S, ld_x, x_al=True, ld_f=None, f_al=True):
    """ola_convtr_impl: the form, its grid.x and, for k_ola_mfma16, the channels per wave / waves with channels / 32-channel batches"""
    m4 = r4(M)
    ok = (K_, S) == (16, 8) and ld_x >= m4 and x_al and (ld_x % 16 == 0 if mode == 1 else ld_x % 4 == 0)
    if mode == 2:
        ok = ok and f_al and ld_f % 4 == 0 and ld_f >= m4
    if not ok:
        return dict(form="generic", gx=cdiv(M + 1, 63))
    cw = cdiv(C, 16) * 4
    return dict(form="mfma", gx=cdiv(M + 1, 60), cw=cw, waves=min(4, cdiv(C, cw)), batches=cdiv(min(cw, C), 32),
                ragged=(C % cw != 0))


def wgrad1_dispatch(N, C, M, coded):
    """frames_wgrad1_launch: the split of the frame range and the passes of the frame loop"""
    fi4 = 16 * (16 if coded else 8)
    msplit = max(1, min(16, cdiv(512, N * cdiv(C, 64))))
    mchunk = cdiv(cdiv(M, msplit), fi4) * fi4
    msplit = cdiv(M, mchunk)
    return dict(msplit=msplit, mchunk=mchunk, passes=cdiv(min(mchunk, M), fi4), last=M - (msplit - 1) * mchunk)


CONV_NAMED = {
    (2, 2, 24, 77, 16, 8): dict(zs=1, co_per=24, co_tile=24, tiles=1, last=24),
    (2, 1, 100, 300, 16, 8): dict(zs=3, co_per=36, co_tile=36, tiles=1, last=28),
    (1, 2, 70, 257, 16, 8): dict(zs=2, co_per=36, co_tile=36, tiles=1, last=34),
    (512, 2, 200, 8, 32, 16): dict(zs=1, co_per=200, co_tile=192, tiles=2, last=200),
    (512, 2, 197, 5, 32, 16): dict(zs=1, co_per=200, co_tile=192, tiles=2, last=197),
    (600, 1, 770, 3, 16, 8): dict(zs=1, co_per=772, co_tile=768, tiles=2, last=770),
}
WG_NAMED = {
    (512, 8, 300): (dict(msplit=1, mchunk=384, passes=3, last=300), dict(msplit=1, mchunk=512, passes=2, last=300)),
    (1, 8, 2100): (dict(msplit=9, mchunk=256, passes=2, last=52), dict(msplit=9, mchunk=256, passes=1, last=52)),
    (1, 8, 4200): (dict(msplit=11, mchunk=384, passes=3, last=360), dict(msplit=9, mchunk=512, passes=2, last=104)),
    (3, 130, 513): (dict(msplit=5, mchunk=128, passes=1, last=1), dict(msplit=3, mchunk=256, passes=1, last=1)),
}


def check_named_dispatch():
    for (N, Ci, Co, M, K_, S), want in CONV_NAMED.items():
        d = conv_dispatch(N, Ci, Co, M, K_, S, (M - 1) * S + K_)
        assert d["form"] == "conv4" and {k: d[k] for k in want} == want, ((N, Ci, Co, M, K_, S), d)
        assert conv_dispatch(N, Ci, Co, M, K_, S, (M - 1) * S + K_ + 1)["form"] == "generic"
    for (N, C, M), (f, c) in WG_NAMED.items():
        assert wgrad1_dispatch(N, C, M, False) == f and wgrad1_dispatch(N, C, M, True) == c, (N, C, M, wgrad1_dispatch(N, C, M, False),
                                                                                           wgrad1_dispatch(N, C, M, True))
    # the decoder's channel split: waves past C (empty), ragged, more than one 32-channel batch
    d = {C: ola_dispatch(0, C, 60, 16, 8, 64) for C in (1, 3, 4, 5, 16, 17, 20, 33, 130)}
    assert [d[C]["waves"] for C in (1, 3, 4, 5, 16, 17, 20, 33, 130)] == [1, 1, 1, 2, 4, 3, 3, 3, 4]
    assert d[130]["batches"] == 2 and d[33]["cw"] == 12 and d[17]["ragged"] and not d[16]["ragged"]
    assert ola_dispatch(0, 4, 60, 16, 8, 65)["form"] == "generic" and ola_dispatch(1, 4, 60, 16, 8, 68)["form"] == "generic"
    assert ola_dispatch(0, 4, 59, 16, 8, 64)["gx"] == 1 and ola_dispatch(0, 4, 60, 16, 8, 64)["gx"] == 2
    assert ola_dispatch(0, 4, 62, 32, 16, 64)["gx"] == 1 and ola_dispatch(0, 4, 63, 32, 16, 64)["gx"] == 2


# ====================================================================================================== references (float64, CPU)
def frames(x, K_, S, M):
    """x [N][Ci][T] -> [N][Ci][M][K]: frame m is x[.., m S : m S + K]"""
    return x.unfold(2, K_, S)[:, :, :M]


def conv_ref(x, w, S, M, add=None):
    """z[n][co][m] = sum_{ci,k} w[co][ci][k] x[n][ci][m S + k] (+ add)"""
    z = torch.einsum("oik,nimk->nom", w.double(), frames(x.double(), w.shape[2], S, M))
    return z + add.double() if add is not None else z


def conv_mag(x, w, S, M, add=None):
    z = torch.einsum("oik,nimk->nom", w.double().abs(), frames(x.double().abs(), w.shape[2], S, M))
    return z + add.double().abs() if add is not None else z


def ola_ref(x, w, S):
    """out[n][t] = sum_c sum_{m S + k = t} x[n][c][m] w[c][k]; x [N][C][M], w [C][K]"""
    N, C, M = x.shape
    K_ = w.shape[1]
    P = torch.einsum("ncm,ck->nmk", x.double(), w.double())
    out = torch.zeros(N, (M - 1) * S + K_, dtype=F64)
    idx = (torch.arange(M)[:, None] * S + torch.arange(K_)[None, :]).reshape(-1)
    return out.index_add_(1, idx, P.reshape(N, -1))


def wgrad_ref(a, x, K_, S):
    """gw[c][ci][k] = sum_{n,m} a[n][c][m] x[n][ci][m S + k]; a [N][C][M], x [N][Ci][T]"""
    return torch.einsum("ncm,nimk->cik", a.double(), frames(x.double(), K_, S, a.shape[2]))


def dec(c, lo, hi):
    """the coded operand's values in float64: delta c + lo with the fp32 step"""
    return delta32(lo, hi).double() * c.double() + f32(lo).double()


def dec32(c, lo, hi):
    """... as the kernels form them: delta * c + lo in two fp32 roundings (fqss_decode)"""
    return delta32(lo, hi) * c.float() + f32(lo)


# ======================================================================================================================= 1. splitter
def split_raw_emul(x):
    """process.preprocess(x, n_splitter=2, normalize=False) in float32, op for op (process.py:26-36): x [B][T] -> [B][2][T]"""
    x = x.unsqueeze(1)
    thr = torch.maximum(x.min().abs(), x.max().abs())
    delta = thr / 128
    q = lambda t: torch.clip(torch.floor(t / delta), -128, 127) * delta
    x0 = q(x)
    x1 = q(2 * (x - x0) * thr / delta - thr)
    return torch.cat([x0, x1], dim=1)


def split_rows_emul(x):
    """the per-item form: process.preprocess on each row alone"""
    return torch.cat([O.split(x[b:b + 1], 2) for b in range(x.shape[0])])


def split_inputs(B, T, seed, level=0.3):
    """a waveform with a DC offset, and -- where they fit -- values on bin edges (multiples of thr / 128), thr itself and -thr, +-0 and
    denormals"""
    g = gen(seed)
    x = torch.randn(B, T, generator=g) * level + 0.1 * level
    thr = float(x.abs().max()) * 1.5
    edge = [thr, -thr, 0.0, -0.0, 1e-40, -1e-40, 1.4e-45, thr / 128, -thr / 128, 5 * thr / 128, thr * 127 / 128, -thr * 127 / 128, thr / 256,
            thr * (1 - 2.0 ** -24), -3 * thr / 128, thr / 128 / 128, 77 * thr / 128]
    flat = x.view(-1)
    n = min(len(edge), flat.numel())
    if flat.numel() == 1:
        return x
    flat[:n] = torch.tensor(edge[:n])
    if n < len(edge):
        flat[0] = thr if flat.numel() > 0 else flat[0]
    return x


def bits_equal(a, b):
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def splitter_run(entry, x):
    """x [B][T] through fqss_splitter2 / _raw (global threshold from fqss_obs_reset + fqss_minmax) or _rows -> out [B][2][T]"""
    B, T = x.shape
    xb, out = Blk(B, T, T, off=1, fill=x), Blk(2 * B, T, T, off=3)
    if entry == "fqss_splitter2_rows":
        ws = torch.zeros(B + 2, dtype=torch.int32, device=L.DEV)
        ws[B:] = 12345
        call(entry, xb.ptr, out.ptr, B, T, ws.data_ptr(), stream())
        assert bits_equal(ws[:B].view(torch.float32).cpu(), x.abs().max(1).values) and bool((ws[B:] == 12345).all()), "row_max"
    else:
        ws = torch.zeros(4, dtype=torch.int32, device=L.DEV)
        call("fqss_obs_reset", ws.data_ptr(), 1, stream())
        call("fqss_minmax", xb.ptr, B, T, T, ws.data_ptr(), stream())
        before = ws.clone()
        call(entry, xb.ptr, out.ptr, B, T, ws.data_ptr(), stream())
        assert bool(torch.equal(ws, before)), "obs_ws changed"
    all_unchanged(x=xb)
    got = out.cpu(B, 2, T)
    nan_ok = bool(torch.isnan(out.buf[:out.o]).all()) and bool(torch.isnan(out.buf[out.o + 2 * B * T:]).all())
    assert nan_ok, f"{entry} wrote outside [B][2][T]"
    return got


SPLIT_SHAPES = [(1, 1), (3, 255), (2, 257), (5, 4096 * 256 // 5 + 3)]      # the last: above 4096 x 256 elements (the grid-stride loop)


def splitter_mutations(x, want, emul_round, tag):
    differs(emul_round, want, "round instead of floor", tag)


def split_round(x, raw=False):
    """the wrong splitter: round to nearest where the reference floors"""
    x = x.unsqueeze(1)
    thr = torch.maximum(x.min().abs(), x.max().abs())
    if not raw:
        x, thr = x / thr, torch.tensor(1.0)
    delta = thr / 128
    q = lambda t: torch.clip(torch.round(t / delta), -128, 127) * delta
    x0 = q(x)
    return torch.cat([x0, q(2 * (x - x0) * thr / delta - thr)], dim=1)


def splitter_body(shapes=SPLIT_SHAPES):
    for k, (B, T) in enumerate(shapes):
        x = split_inputs(B, T, 10 + k)
        for entry, want in (("fqss_splitter2", O.split(x, 2)), ("fqss_splitter2_raw", split_raw_emul(x))):
            if not have(entry):
                continue
            got = splitter_run(entry, x)
            assert bits_equal(got, want), (entry, B, T, int((got != want).sum()))
            if B * T > 16:
                differs(split_round(x, raw=entry.endswith("raw")), want, "round instead of floor", f"{entry} {B} x {T}")
            assert bool(torch.isfinite(got).all())
        if B * T > 1:
            thr = float(x.abs().max())
            got = splitter_run("fqss_splitter2", x) if have("fqss_splitter2") else None
            if got is not None:
                assert float(got[:, 0].max()) == 127 / 128 and float(got[:, 0].min()) == -1.0, "thr clamps to 127, -thr is -128"
                assert thr > 0


def splitter_rows_body(long_row=True):
    g = gen(3)
    T = 300
    x = torch.randn(5, T, generator=g) * 0.3 + 0.05
    x = x * torch.tensor([1.0, 1e-3, 7.0, 1e-30, 1.0])[:, None]
    x[:, :6] = x.abs().max(1).values[:, None] * torch.tensor([1.0, -1.0, 1 / 128, 0.0, -0.0, 77 / 128])[None]
    x[4] = 0.0                                                       # the silent row
    x[4, 1] = -0.0
    want = split_rows_emul(x)
    got = splitter_run("fqss_splitter2_rows", x)
    assert bool(torch.isnan(want[4]).all()) and bool(torch.isfinite(want[:4]).all())
    assert bool(torch.isnan(got[4]).all()), "a silent row is NaN in that row"
    assert bits_equal(got[:4], want[:4]), "rows beside the silent one"
    differs(O.split(x[:4], 2), want[:4], "the global threshold where the row threshold belongs", "splitter rows")
    differs(torch.cat([split_round(x[b:b + 1]) for b in range(4)]), want[:4], "round instead of floor", "splitter rows")
    for B, T in [(1, 1), (3, 255), (2, 257)] + ([(2, 1024 * 256 + 257)] if long_row else []):
        # the last: grid_rows(B, T, 1, 1024) is 1024 x 1 workgroups -- both loops of k_row_absmax / k_splitter2_rows wrap
        x = split_inputs(B, T, 20 + B) * torch.tensor([1.0, 0.01, 30.0][:B])[:, None]
        got, want = splitter_run("fqss_splitter2_rows", x), split_rows_emul(x)
        assert bits_equal(got, want), (B, T, int((got != want).sum()))


@gpu
def test_splitter_bit_for_bit():
    """fqss_splitter2 / _raw against the float32 emulations, bin edges, +-thr, +-0 and denormals included; one case in the grid-stride loop"""
    splitter_body()


@gpu
def test_splitter_rows_bit_for_bit():
    """fqss_splitter2_rows: rows at very different levels against the per-row emulation; a silent row is NaN in that row only"""
    splitter_rows_body()


@gpu
def test_splitter_refusals():
    """every FQSS_REQUIRE of the three splitters; B = 0 and T = 0 are no-ops that write nothing"""
    x, out = Blk(2, 8, 8, fill=torch.ones(2, 8)), Blk(4, 8, 8)
    ws = torch.zeros(4, dtype=torch.int32, device=L.DEV)
    S = stream()
    for e in ("fqss_splitter2", "fqss_splitter2_raw"):
        for a in ((None, out.ptr, 2, 8, ws.data_ptr()), (x.ptr, None, 2, 8, ws.data_ptr()), (x.ptr, out.ptr, 2, 8, None),
                  (x.ptr, out.ptr, -1, 8, ws.data_ptr()), (x.ptr, out.ptr, 2, -1, ws.data_ptr())):
            refused(e, *a, S)
        call(e, x.ptr, out.ptr, 0, 8, ws.data_ptr(), S)
        call(e, x.ptr, out.ptr, 2, 0, ws.data_ptr(), S)
    for a in ((None, out.ptr, 2, 8, ws.data_ptr()), (x.ptr, None, 2, 8, ws.data_ptr()), (x.ptr, out.ptr, 2, 8, None),
              (x.ptr, out.ptr, 0, 8, ws.data_ptr()), (x.ptr, out.ptr, 2, 0, ws.data_ptr())):
        refused("fqss_splitter2_rows", *a, S)
    assert out.untouched() and x.unchanged() and bool((ws == 0).all())


# =================================================================================================================== 2. framing conv
# (N, Ci, Co, M, K, S, tail): T = (M - 1) S + K + tail -- the signal has `tail` samples that no frame covers
CONV_CASES = [(2, 2, 24, 77, 16, 8, 0), (2, 1, 100, 300, 16, 8, 4), (1, 2, 70, 257, 16, 8, 0), (512, 2, 200, 8, 32, 16, 0),
              (512, 2, 197, 5, 32, 16, 8), (600, 1, 770, 3, 16, 8, 0),
              (3, 1, 1, 1, 16, 8, 0), (2, 2, 3, 3, 32, 16, 4), (1, 1, 5, 4, 16, 8, 12), (1, 2, 5, 5, 16, 8, 0), (2, 1, 33, 255, 32, 16, 0),
              (1, 2, 8, 256, 16, 8, 8), (1, 1, 3, 257, 32, 16, 0),
              (2, 1, 7, 130, 2, 1, 3), (3, 2, 33, 65, 2, 1, 0)]                 # the generic-only (K, S) = (2, 1)
CONV_FORMS = ("xoff", "todd", "ldodd", "zoff", "short")


def conv_operands(case, mode, seed):
    """mode "int": integers (|x| <= 15, |w| <= 15, |add| <= 1000); "real": a waveform with a DC offset, heavy-tailed taps"""
    N, Ci, Co, M, K_, S, tail = case
    g = gen(seed)
    T = (M - 1) * S + K_ + tail
    if mode == "int":
        return ints(g, 15, N, Ci, T), ints(g, 15, Co, Ci, K_), ints(g, 1000, N, Co, M)
    x = torch.randn(N, Ci, T, generator=g) * 0.2 + 0.15
    return x, torch.randn(Co, Ci, K_, generator=g) * (Ci * K_) ** -0.5, torch.randn(N, Co, M, generator=g) * 0.3


def conv_run(x, w, S, M, form, add=None, add_form="al", big=False):
    """one call of fqss_frames_conv_fwd / _add_fwd; form "c4": every operand eligible for k_frames_conv4, else one disqualifier.
    Returns z [N][Co][M] and the form the mirror of the launch code expects; asserts the written region of that form"""
    N, Ci, T = x.shape
    Co, _, K_ = w.shape
    m4 = r4(M)
    if form == "todd":                                   # tail samples that no frame covers: the same live values, T % 4 != 0
        x = torch.cat([x, torch.full((N, Ci, 1 + M % 3), 3.0)], 2) if (T + 1 + M % 3) % 4 else torch.cat([x, torch.full((N, Ci, 1), 3.0)], 2)
        T = x.shape[2]
        assert T % 4
    xb = Blk(N * Ci, T, T, off=1 if form == "xoff" else 0, fill=x)
    wb = Blk(Co, Ci * K_, Ci * K_, off=2, fill=w)
    ex = 0 if big else 8
    ld_z = {"ldodd": m4 + ex + 1, "short": M}.get(form, m4 + ex)
    z = Blk(N * Co, M, ld_z, off=1 if form == "zoff" else 0)
    ab, ld_add = None, None
    if add is not None:
        ld_add = {"odd": m4 + 5, "short": M}.get(add_form, m4 + 4)
        ab = Blk(N * Co, M, ld_add, off=1 if add_form == "off" else 0, fill=add)
        assert ld_add != ld_z
    d = conv_dispatch(N, Ci, Co, M, K_, S, T, x_al=form != "xoff", z_al=form != "zoff", ld_z=ld_z, add_al=add_form != "off", ld_add=ld_add)
    if add is None:
        call("fqss_frames_conv_fwd", xb.ptr, wb.ptr, z.ptr, N, Ci, Co, T, K_, S, M, ld_z, stream())
    else:
        call("fqss_frames_conv_add_fwd", xb.ptr, wb.ptr, ab.ptr, ld_add, z.ptr, N, Ci, Co, T, K_, S, M, ld_z, stream())
        all_unchanged(add=ab)
    all_unchanged(x=xb, w=wb)
    if d["form"] == "conv4" and on_gpu():
        assert fwritten(z), "k_frames_conv4 wrote beyond column roundup4(M) of a row (or left a live element)"
    else:
        assert z.written(), "the generic framing conv wrote outside [0, M) (or left a live element)"
    return z.cpu(N, Co, M), d["form"]


def conv_forms(case, k):
    """the aligned form and two disqualifiers by turns (the big shapes: one)"""
    N, Ci, Co, M, K_, S, tail = case
    big = N * Co * M > 500000
    if (K_, S) == (2, 1):
        return ["c4", "ldodd"], big
    fs = [CONV_FORMS[k % 5]] if big else [CONV_FORMS[k % 5], CONV_FORMS[(k + 2) % 5]]
    return ["c4"] + [f for f in fs if not (f == "short" and M % 4 == 0)] + (["xoff"] if M % 4 == 0 and not big and "xoff" not in fs else []), big


def conv_body(case, mode, with_add=True):
    """every form of the case, without and with the addend: the forms agree bit for bit; "int": equal to the integer sums, "real": every
    element within the derived bound of float64"""
    k = CONV_CASES.index(case)
    N, Ci, Co, M, K_, S, tail = case
    x, w, add = conv_operands(case, mode, 1000 + k)
    forms, big = conv_forms(case, k)
    tag = f"conv {mode} {case}"
    fails = []
    for a in ((None, add) if with_add and have("fqss_frames_conv_add_fwd") else (None,)):
        ref, mag = conv_ref(x, w, S, M, a), conv_mag(x, w, S, M, a)
        if mode == "int":
            assert exact_ok(mag), tag
        outs = {}
        for f in forms:
            outs[f], took = conv_run(x, w, S, M, f, add=a, big=big)
            assert not on_gpu() or took == ("conv4" if f == "c4" and (K_, S) != (2, 1) else "generic"), (tag, f, took)
        if a is not None and not big:
            for af in ("off", "odd") + (("short",) if M % 4 else ()):
                outs["add" + af], took = conv_run(x, w, S, M, "c4", add=a, add_form=af)
                assert not on_gpu() or took == "generic"
        z0 = outs["c4"]
        for f, z in outs.items():
            assert torch.equal(z, z0), (tag, f, "the forms of the framing conv differ", int((z != z0).sum()))
        n = Ci * K_
        bnd = (n + 2) * ULP * mag
        if mode == "int":
            assert torch.equal(z0, ref.float()), (tag, a is not None, int((z0 != ref.float()).sum()))
        else:
            z32 = F.conv1d(x, w, stride=S)[:, :, :M] + (a if a is not None else 0)
            worst = float(((z0.double() - ref).abs() / bnd).max())
            worst32 = float(((z32.double() - ref).abs() / bnd).max())
            e = errs(z0, ref)
            print(f"MEAS conv z {worst:.2f} of the element's bound (e_elem {e[0]:.2e} e_norm {e[1]:.2e}), torch fp32 {worst32:.2f} | {tag} add={a is not None}")
            if not worst <= 1.0:
                fails.append((tag, worst))
        conv_mutations(x, w, S, M, a, ref, bnd, mode, tag, fails)
    assert not fails, fails


def unit_floor(mut, ref, bnd, what, tag, fails, mode):
    """framing conv: the wrong kernel misses the derived per-element bound by 10 x somewhere (exact cases: elements that differ)"""
    if mode == "int":
        differs(mut, ref, what, tag)
        return
    fl = float(((mut - ref).abs() / bnd.clamp_min(1e-300)).max())
    print(f"FLOOR conv z {what} {fl:.2e} x the element's bound | {tag}")
    if not fl >= 10:
        fails.append(("floor", tag, what, fl))


def conv_mutations(x, w, S, M, add, ref, bnd, mode, tag, fails):
    N, Ci, T = x.shape
    Co, _, K_ = w.shape
    mut = ref.clone()
    mut[:, :, M - 1] = add[:, :, M - 1].double() if add is not None else 0.0
    unit_floor(mut, ref, bnd, "last frame dropped", tag, fails, mode)
    if Ci > 1:
        unit_floor(conv_ref(x[:, :1], w[:, :1], S, M, add), ref, bnd, "last channel dropped", tag, fails, mode)
    if Co > 1:
        unit_floor(conv_ref(x, w.roll(1, 0), S, M, add), ref, bnd, "a tap row of the neighbouring channel", tag, fails, mode)
    if M > 1:
        unit_floor(conv_ref(x, w, S, M, None).roll(1, 2) + (add.double() if add is not None else 0.0), ref, bnd, "frame index one off", tag,
                   fails, mode)
    unit_floor(conv_ref(x[:, :, :T - 1], w[:, :, :K_ - 1], S, M, add) if T - 1 >= (M - 1) * S + K_ - 1 else ref * 0, ref, bnd,
               "last tap dropped", tag, fails, mode)
    if add is not None:
        unit_floor(conv_ref(x, w, S, M), ref, bnd, "the addend dropped", tag, fails, mode)
        # ld_add read as ld_z = ld_add + 4: element (row, m) comes from flat position row (ld_add + 4) + m of the addend's rows
        ld_add = r4(M) + 4
        flat = torch.full((N * Co * (ld_add + 4) + 8,), rms(add), dtype=F64)
        flat[:N * Co * ld_add].view(N * Co, ld_add)[:, :M] = add.double().reshape(N * Co, M)
        wrong = flat[:N * Co * (ld_add + 4)].view(N * Co, ld_add + 4)[:, :M].reshape(N, Co, M)
        if N * Co > 1:
            unit_floor(conv_ref(x, w, S, M) + wrong, ref, bnd, "ld_add read as ld_z", tag, fails, mode)


@gpu
@pytest.mark.parametrize("case", CONV_CASES, ids=str)
def test_frames_conv_exact_integers(case):
    """fqss_frames_conv_fwd / _add_fwd on integers: k_frames_conv4 and k_frames_conv_fwd equal the integer sums bit for bit"""
    conv_body(case, "int")


@gpu
@pytest.mark.parametrize("case", CONV_CASES, ids=str)
def test_frames_conv_against_fp64(case):
    """real operands with a DC offset: every element within (Ci K + 2) 2^-24 sum |x w| of float64; the two forms agree bit for bit"""
    conv_body(case, "real")


@gpu
def test_frames_conv_refusals():
    """every FQSS_REQUIRE / set_error of frames_conv_impl through both entries; z is untouched; N = 0 and M = 0 are no-ops"""
    N, Ci, Co, M, K_, S = 2, 1, 3, 5, 16, 8
    T = (M - 1) * S + K_
    x, w, add = Blk(N * Ci, T, T, fill=torch.ones(N, T)), Blk(Co, K_, K_, fill=torch.ones(Co, K_)), Blk(N * Co, M, 12, fill=torch.ones(N * Co, M))
    z = Blk(N * Co, M, 8)
    St = stream()
    who = "frames_conv_impl"

    def both(x_=x.ptr, w_=w.ptr, z_=z.ptr, N=N, Ci=Ci, Co=Co, T=T, K_=K_, S=S, M=M, ldz=8, ldadd=12, who=who):
        refused("fqss_frames_conv_fwd", x_, w_, z_, N, Ci, Co, T, K_, S, M, ldz, St, who=who)
        refused("fqss_frames_conv_add_fwd", x_, w_, add.ptr, ldadd, z_, N, Ci, Co, T, K_, S, M, ldz, St, who=who)

    for k in ("x_", "w_", "z_"):
        both(**{k: None})
    both(N=-1)
    both(N=65536)
    both(Ci=0)
    both(Co=0)
    both(K_=0)
    both(S=0)
    both(M=-1)
    both(ldz=4)                                              # ld_z < M
    both(T=T - 1)                                            # frames exceed the signal
    both(Ci=3, T=T, who="unsupported (Ci=3")                 # set_error of the dispatch: the entry's own name in front
    both(K_=8, who="unsupported (Ci=1, K=8")
    refused("fqss_frames_conv_add_fwd", x.ptr, w.ptr, None, 12, z.ptr, N, Ci, Co, T, K_, S, M, 8, St)                      # null addend
    refused("fqss_frames_conv_add_fwd", x.ptr, w.ptr, add.ptr, 4, z.ptr, N, Ci, Co, T, K_, S, M, 8, St, who=who)           # ld_add < M
    assert z.untouched()
    for n_, m_ in ((0, M), (N, 0)):
        call("fqss_frames_conv_fwd", x.ptr, w.ptr, z.ptr, n_, Ci, Co, T, K_, S, m_, 8, St)
        call("fqss_frames_conv_add_fwd", x.ptr, w.ptr, add.ptr, 12, z.ptr, n_, Ci, Co, T, K_, S, m_, 8, St)
    assert z.untouched()
    all_unchanged(x=x, w=w, add=add)


# ======================================================================================================================== 3. decoder
# (N, C, M, K, S): C makes the per-wave channel split of k_ola_mfma16 empty (waves past C), ragged and longer than one 32-channel batch;
# M sits around the 60-slot workgroup of the matrix-core form and the 63-slot one of the generic form
DEC_CASES = [(1, 1, 1, 16, 8), (3, 3, 2, 16, 8), (1, 4, 3, 16, 8), (3, 5, 4, 16, 8), (1, 16, 59, 16, 8), (3, 17, 60, 16, 8), (1, 20, 61, 16, 8),
             (3, 33, 119, 16, 8), (1, 130, 120, 16, 8), (3, 130, 121, 16, 8), (1, 5, 62, 32, 16), (3, 33, 63, 32, 16), (1, 130, 64, 32, 16),
             (3, 17, 62, 2, 1), (1, 4, 63, 2, 1), (3, 1, 64, 2, 1)]
LO, HI = -0.731, 1.913                       # the coded operand's range in the float64 cases
ILO = -100.0                                 # ... in the exact cases: [lo, lo + 255], delta = 1


def fam_of(form):
    return "ola_mfma" if form == "mfma" else "ola_gen"


def xlay(M, kind, coded=False, extra=4):
    """(ld, offset) of decoder / wgrad operand rows: "al" vector-aligned with padding beyond the round-up; "odd" a row stride that
    disqualifies the matrix-core form (fp32: ld % 4 == 1; codes: ld % 16 == 4); "off" the base one element off"""
    if coded:
        return {"al": (r16(M) + 16, 0), "odd": (r16(M) + 4, 0), "off": (r16(M) + 16, 1), "min": (r16(M), 0)}[kind]
    return {"al": (r4(M) + extra, 0), "odd": (r4(M) + extra + 1, 0), "off": (r4(M) + extra, 1), "min": (r4(M), 0)}[kind]


def ola_run(mode, x, w, S, kind, feat=None, NS=1, lo=None, hi=None, fkind=None):
    """one decoder call.  mode 0: x fp32 [N][C][M]; 1: x u8 codes of (lo, hi); 2: x = mask [N][C][M], feat [N / NS][C][M].  Returns out
    [N][T] and the form the mirror of the launch code expects"""
    N, C, M = x.shape
    K_ = w.shape[1]
    T = (M - 1) * S + K_
    ld, off = xlay(M, kind, coded=mode == 1)
    xb = (Cod if mode == 1 else Blk)(N * C, M, ld, off=off, fill=x)
    wb = Blk(C, K_, K_, off=1, fill=w)
    out = Blk(N, T, T, off=2)
    ops = dict(x=xb, w=wb)
    ld_f, f_al = None, True
    if mode == 0:
        call("fqss_ola_convtr_fwd", xb.ptr, wb.ptr, out.ptr, N, C, M, ld, K_, S, T, stream())
    elif mode == 1:
        qlo, qhi = sc(lo), sc(hi)
        ops.update(lo=qlo, hi=qhi)
        call("fqss_ola_convtr_fwd_q", xb.ptr, qlo.ptr, qhi.ptr, wb.ptr, out.ptr, N, C, M, ld, K_, S, T, stream())
    else:
        fkind = fkind or kind
        ld_f, foff = xlay(M, fkind, extra=12)
        f_al = foff == 0
        fb = Blk(N // NS * C, M, ld_f, off=foff, fill=feat)
        ops.update(feat=fb)
        assert ld_f != ld
        call("fqss_ola_convtr_mul_fwd", xb.ptr, fb.ptr, wb.ptr, out.ptr, N, NS, C, M, ld, ld_f, K_, S, T, stream())
    all_unchanged(**ops)
    assert out.written(), "the decoder wrote outside [0, T) of out (or left a live element)"
    d = ola_dispatch(mode, C, M, K_, S, ld, x_al=off == 0, ld_f=ld_f, f_al=f_al)
    return out.cpu(N, T), d["form"]


def decode_run(c, lo, hi, kind):
    """fqss_decode of the codes into fp32 rows of layout `kind` -> the CPU values (the unfused chain's intermediate)"""
    N, C, M = c.shape
    cb = Cod(N * C, M, r16(M), fill=c)
    ld, off = xlay(M, kind)
    xb = Blk(N * C, M, ld, off=off)
    qlo, qhi = sc(lo), sc(hi)
    call("fqss_decode", cb.ptr, xb.ptr, N * C, M, cb.ld, ld, qlo.ptr, qhi.ptr, stream())
    assert fwritten(xb)           # (fqss_decode stores whole float4s into the row padding: its own contract, not this file's)
    return xb.cpu(N, C, M)


def mul_run(mask, feat, NS):
    N, C, M = mask.shape
    mb, fb = Blk(N * C, M, r4(M) + 4, fill=mask), Blk(N // NS * C, M, r4(M) + 8, fill=feat)
    z = Blk(N * C, M, r4(M))
    call("fqss_mul_bcast_fwd", mb.ptr, fb.ptr, z.ptr, N // NS, NS, C, M, mb.ld, fb.ld, z.ld, stream())
    assert z.written()
    return z.cpu(N, C, M)


def dec_operands(case, mode, seed, NS=1):
    """(x, w, codes, mask, feat) of a decoder case; N of the masking form is NS x the case's N"""
    N, C, M, K_, S = case
    g = gen(seed)
    if mode == "int":
        x, w = ints(g, 8, N, C, M), ints(g, 8, C, K_)
        c = torch.randint(80, 121, (N, C, M), generator=g, dtype=torch.uint8)           # values -20 .. 20 under ILO
        mask, feat = ints(g, 3, N * NS, C, M), ints(g, 3, N, C, M)
    else:
        x, w = torch.randn(N, C, M, generator=g) * 0.5 + 0.2, torch.randn(C, K_, generator=g) * C ** -0.5 + 0.05
        c = codes(g, N, C, M)
        mask, feat = torch.rand(N * NS, C, M, generator=g), torch.randn(N, C, M, generator=g) * 0.5 + 0.2
    return x, w, c, mask, feat


def kinds_for(case, k):
    N, C, M, K_, S = case
    return ("al", "odd", "off") if k % 2 == 0 else ("al", "odd")


def ola_mutations(fam, x64, w, S, ref, tag, fails, mode):
    """x64: the operand's values in float64 [N][C][M]"""
    N, C, M = x64.shape
    K_ = w.shape[1]

    def fl(mut, what):
        if mode == "int":
            differs(mut, ref, what, tag)
        else:
            floor(fam, "out", mut, ref, what, tag, fails)

    x0 = x64.clone()
    x0[:, :, M - 1] = 0
    fl(ola_ref(x0, w, S), "last frame dropped")
    if C > 1:
        fl(ola_ref(x64[:, :C - 1], w[:C - 1], S), "last channel dropped")
        fl(ola_ref(x64, w.roll(1, 0), S), "a tap row of the neighbouring channel")
    if C > 4:
        cw = cdiv(C, 16) * 4
        keep = torch.ones(C, dtype=torch.bool)
        if fam == "ola_mfma":
            keep[cw:2 * cw] = False
        else:
            keep[1::4] = False
        fl(ola_ref(x64[:, keep], w[keep], S), "one wave's channel block dropped")
    if M > 1:
        fl(ola_ref(x64.roll(1, 2), w, S), "frame index one off")
        w0 = w.double().clone()
        w0[:, S:] = 0
        mut = ola_ref(x64, w0, S)
        mut[:, (M - 1) * S + S:] = ref[:, (M - 1) * S + S:]
        mut[:, :S] = ref[:, :S]
        fl(mut, "the overlap term (r = 1) dropped")
    # padding column M read as a value of the rms: frame M lands on the slots it shares with [0, T)
    # (against |w|: integer taps can sum to zero over the channels)
    xe = torch.cat([x64, rms(x64) * torch.sign(w.double()[:, 0] + 0.5)[None, :, None].expand(N, C, 1)], 2)
    fl(ola_ref(xe, w, S)[:, :ref.shape[1]], "padding column M read as a value of the rms")


def dec_body(case, mode, modes=(0, 1, 2)):
    """all three operand modes in both forms.  "int": every form equals the integer sums; "real": each form against float64, the pair
    within the sum of the bounds; the fused forms bit-identical to their unfused chains where both take the same form"""
    k = DEC_CASES.index(case)
    N, C, M, K_, S = case
    NS = (1, 2, 3)[k % 3]
    x, w, c, mask, feat = dec_operands(case, mode, 2000 + k, NS)
    lo, hi = (ILO, ILO + 255.0) if mode == "int" else (LO, HI)
    fails = []
    tag0 = f"ola {mode} {case}"
    T = (M - 1) * S + K_
    for md in modes:
        entry = ("fqss_ola_convtr_fwd", "fqss_ola_convtr_fwd_q", "fqss_ola_convtr_mul_fwd")[md]
        if not have(entry):
            continue
        if md == 0:
            x64, x32, args = x.double(), x, dict()
        elif md == 1:
            x64, x32, args = dec(c, lo, hi), dec32(c, lo, hi), dict(lo=lo, hi=hi)
        else:
            fx = feat.repeat_interleave(NS, 0)
            x64, x32, args = mask.double() * fx.double(), mask * fx, dict(feat=feat, NS=NS)
        ref = ola_ref(x64, w, S)
        if mode == "int":
            assert float(delta32(lo, hi)) == 1.0 and exact_ok(ola_ref(x64.abs(), w.abs(), S)), tag0
        r32 = F.conv_transpose1d(x32, w[:, None, :], stride=S)[:, 0]
        src = (x, c, mask)[md]
        outs = {}
        for kind in kinds_for(case, k):
            got, form = ola_run(md, src, w, S, kind, **args)
            assert got.shape == (N * (NS if md == 2 else 1), T)
            if on_gpu():
                assert form == ("mfma" if kind == "al" and (K_, S) == (16, 8) else "generic"), (tag0, md, kind, form)
            tag = f"{tag0} mode {md} {kind} ({form})"
            if mode == "int":
                assert torch.equal(got, ref.float()), (tag, int((got != ref.float()).sum()))
            else:
                measure(fam_of(form), "out", got, ref, r32, tag, fails)
            outs[kind] = (got, form)
        if md == 2 and on_gpu():                          # the feature operand alone disqualifies the matrix-core form
            got, form = ola_run(2, mask, w, S, "al", feat=feat, NS=NS, fkind="odd")
            assert form == "generic" and torch.equal(got, outs["odd"][0]), (tag0, "feat disqualified")
        for form in {f for _, f in outs.values()}:
            ola_mutations(fam_of(form), x64, w, S, ref, f"{tag0} mode {md}", fails, mode)
        if mode == "real":
            for kind, (got, form) in outs.items():       # the pair of forms within the sum of their bounds
                e = errs(got, outs["al"][0].double())
                b = BOUND[fam_of(form)]["out"][0] + BOUND[fam_of(outs["al"][1])]["out"][0]
                print(f"PAIR ola al vs {kind} e_elem {e[0]:.2e} (equal: {torch.equal(got, outs['al'][0])}) | {tag0} mode {md}")
                if not e[0] * rms(outs["al"][0]) / rms(ref) <= b:
                    fails.append((tag0, md, kind, "pair", e))
        if md in (1, 2) and on_gpu():
            # the unfused chain: fqss_decode / fqss_mul_bcast_fwd into fp32 rows, then fqss_ola_convtr_fwd
            mid = decode_run(c, lo, hi, "al") if md == 1 else mul_run(mask, feat, NS)
            assert torch.equal(mid, x32), (tag0, md, "the unfused chain's intermediate")
            chain = {kd: ola_run(0, mid, w, S, kd) for kd in ("al", "odd")}
            for kd in ("al", "odd"):                      # both calls in the same form: bit-identical
                assert chain[kd][1] == outs[kd][1]
                assert torch.equal(chain[kd][0], outs[kd][0]), (tag0, md, kd, "fused form != unfused chain in the same form")
            # the fused call generic, the chain's decoder on the matrix cores (and the reverse): another summation order
            for kf, kc in (("odd", "al"), ("al", "odd")):
                same = torch.equal(outs[kf][0], chain[kc][0])
                print(f"MIXED mode {md} fused {outs[kf][1]} vs chain {chain[kc][1]}: bit-identical {same} | {tag0}")
                if mode == "int":
                    assert same
    assert not fails, fails


@gpu
@pytest.mark.parametrize("case", DEC_CASES, ids=str)
def test_decoder_exact_integers(case):
    """the three decoder entries on integers (codes with delta = 1): the matrix-core and the generic form equal the integer sums"""
    dec_body(case, "int")


@gpu
@pytest.mark.parametrize("case", DEC_CASES, ids=str)
def test_decoder_against_fp64(case):
    """real operands with a DC offset, each form against float64; fqss_ola_convtr_fwd_q / _mul_fwd bit-identical to fqss_decode /
    fqss_mul_bcast_fwd + fqss_ola_convtr_fwd when both calls take the same form"""
    dec_body(case, "real")


@gpu
def test_decoder_refusals():
    """every FQSS_REQUIRE / set_error of ola_convtr_impl through the three entries; out is untouched; N = 0 and M = 0 are no-ops"""
    N, C, M, K_, S = 2, 3, 5, 16, 8
    T = (M - 1) * S + K_
    x, f, w = Blk(N * C, M, 8, fill=torch.ones(N * C, M)), Blk(N * C, M, 12, fill=torch.ones(N * C, M)), Blk(C, K_, K_, fill=torch.ones(C, K_))
    xc = Cod(N * C, M, 16, fill=torch.zeros(N * C, M, dtype=torch.uint8))
    lo, hi, out = sc(0.0), sc(1.0), Blk(N, T, T)
    St = stream()
    who = "ola_convtr_impl"

    def all3(x_=True, w_=w.ptr, out_=out.ptr, N=N, C=C, M=M, ld=None, K_=K_, S=S, T=T, who=who):
        refused("fqss_ola_convtr_fwd", x.ptr if x_ else None, w_, out_, N, C, M, ld or 8, K_, S, T, St, who=who)
        refused("fqss_ola_convtr_fwd_q", xc.ptr if x_ else None, lo.ptr, hi.ptr, w_, out_, N, C, M, ld or 16, K_, S, T, St, who=who)
        refused("fqss_ola_convtr_mul_fwd", x.ptr if x_ else None, f.ptr, w_, out_, N, 1, C, M, ld or 8, 12, K_, S, T, St, who=who)

    all3(x_=False)
    all3(w_=None)
    all3(out_=None)
    all3(N=-1)
    all3(N=65536)
    all3(C=0)
    all3(M=-1)
    all3(ld=4)                                               # ld_x < M
    all3(K_=0)
    all3(S=0)
    all3(T=T + 1)                                            # T != (M - 1) S + K
    all3(K_=8, S=4, T=(M - 1) * 4 + 8, who="unsupported (K=8, stride=4)")
    refused("fqss_ola_convtr_fwd_q", xc.ptr, None, hi.ptr, w.ptr, out.ptr, N, C, M, 16, K_, S, T, St, who=who)            # no ranges
    refused("fqss_ola_convtr_fwd_q", xc.ptr, lo.ptr, None, w.ptr, out.ptr, N, C, M, 16, K_, S, T, St, who=who)
    mul = lambda f_=f.ptr, NS=1, ldf=12: refused("fqss_ola_convtr_mul_fwd", x.ptr, f_, w.ptr, out.ptr, N, NS, C, M, 8, ldf, K_, S, T, St, who=who)
    mul(f_=None)
    mul(NS=0)
    mul(NS=3)                                                # N % NS != 0
    mul(ldf=4)                                               # ld_f < M
    assert out.untouched()
    for n_, m_ in ((0, M), (N, 0)):
        call("fqss_ola_convtr_fwd", x.ptr, w.ptr, out.ptr, n_, C, m_, 8, K_, S, T, St)
        call("fqss_ola_convtr_fwd_q", xc.ptr, lo.ptr, hi.ptr, w.ptr, out.ptr, n_, C, m_, 16, K_, S, T, St)
        call("fqss_ola_convtr_mul_fwd", x.ptr, f.ptr, w.ptr, out.ptr, n_, 1, C, m_, 8, 12, K_, S, T, St)
    assert out.untouched()
    all_unchanged(x=x, f=f, w=w, xc=xc)


# =============================================================================================================== 4. weight gradients
# (N, C, M, K, S, tail)
WG_CASES = [(2, 1, 1, 16, 8, 0), (1, 15, 7, 32, 16, 4), (3, 16, 8, 16, 8, 0), (2, 17, 9, 32, 16, 0), (1, 63, 127, 16, 8, 8),
            (2, 64, 128, 32, 16, 0), (1, 65, 129, 16, 8, 0), (2, 130, 255, 32, 16, 4), (1, 16, 256, 16, 8, 0), (2, 15, 257, 32, 16, 0),
            (512, 8, 300, 16, 8, 0), (1, 8, 2100, 32, 16, 0), (1, 8, 4200, 16, 8, 4), (3, 130, 513, 16, 8, 0)]
WG21_CASES = [(2, 5, 130, 2, 1, 3), (1, 33, 65, 2, 1, 0)]          # fqss_frames_wgrad alone: (K, S) = (2, 1)


def wg_operands(case, mode, seed, Ci=1):
    """a [N][C][M] (fp32) and its coded counterpart, the signal x [N][Ci][T], the start of gw [C][Ci][K]"""
    N, C, M, K_, S, tail = case
    g = gen(seed)
    T = (M - 1) * S + K_ + tail
    if mode == "int":
        la = 8 if N * M < 20000 else 2
        a, x = ints(g, la, N, C, M), ints(g, 7, N, Ci, T)
        c = torch.randint(100 - la, 100 + la + 1, (N, C, M), generator=g, dtype=torch.uint8)       # values -la .. la under ILO
        start = ints(g, 1000, C, Ci, K_)
    else:
        a, x = heavy(g, N, C, M), torch.randn(N, Ci, T, generator=g) * 0.2 + 0.15
        c = codes(g, N, C, M)
        start = None
    return a, c, x, start


def real_start(ref, seed):
    return (torch.randn(ref.shape, generator=gen(seed)) * rms(ref)).float()


def wg_run(entry, a, x, start, K_, S, kind="al", ci=None, lo=None, hi=None, expect=0):
    """one weight-gradient call into a gw that starts from `start` [C][Ci][K].  entry fqss_frames_wgrad: every channel of x; _wgrad1 / _q:
    x has one channel; _wgrad1s: channel ci of x into column block ci of gw (rows ld_gw = Ci K + 4 apart).  Returns gw [C][Ci][K]"""
    N, C, M = a.shape
    _, Ci, T = x.shape
    coded = entry.endswith("_q")
    ld, off = xlay(M, kind, coded=coded, extra=8)
    ab = (Cod if coded else Blk)(N * C, M, ld, off=off, fill=a)
    xb = Blk(N * Ci, T, T, off=0 if kind == "al" else 3, fill=x)      # (launch_gemm's vector loads need the signal aligned too)
    ld_gw = Ci * K_ + (4 if entry.endswith("1s") else 0)
    gw = Blk(C, Ci * K_, ld_gw, off=1, fill=start)
    ops = dict(a=ab, x=xb)
    St = stream()
    if entry == "fqss_frames_wgrad":
        args = (ab.ptr, xb.ptr, gw.ptr, N, C, Ci, M, ld, T, K_, S, St)
    elif entry == "fqss_frames_wgrad1":
        args = (ab.ptr, xb.ptr, gw.ptr, N, C, M, ld, T, K_, S, St)
    elif entry == "fqss_frames_wgrad1s":
        args = (ab.ptr, xb.ptr + 4 * ci * T, Ci * T, gw.ptr + 4 * ci * K_, ld_gw, N, C, M, ld, T, K_, S, St)
    else:
        qlo, qhi = sc(lo), sc(hi)
        ops.update(lo=qlo, hi=qhi)
        args = (ab.ptr, qlo.ptr, qhi.ptr, xb.ptr, gw.ptr, N, C, M, ld, T, K_, S, St)
    if expect:
        refused(entry, *args)
        assert gw.unchanged(), "a refused weight gradient touched gw"
        return None
    call(entry, *args)
    all_unchanged(**ops)
    assert gw.written(), f"{entry} wrote outside the C x K of gw"
    got = gw.cpu(C, Ci, K_)
    if ci is not None and Ci > 1:
        other = [i for i in range(Ci) if i != ci]
        assert bits_equal_f(got[:, other], start[:, other]), "fqss_frames_wgrad1s touched another column block of gw"
    return got


def bits_equal_f(a, b):
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def wg_mutations(fam, a64, x, K_, S, ref, tag, fails, mode, split=None, lo_term=None):
    N, C, M = a64.shape
    T = x.shape[2]

    def fl(mut, what):
        if mode == "int":
            differs(mut, ref, what, tag)
        else:
            floor(fam, "gw", mut, ref, what, tag, fails)

    a0 = a64.clone()
    a0[:, :, M - 1] = 0
    fl(wgrad_ref(a0, x, K_, S), "last frame dropped")
    if M > 1:
        fl(wgrad_ref(a64.roll(1, 2), x, K_, S), "frame index one off")
    if C > 1:
        fl(wgrad_ref(a64.roll(1, 1), x, K_, S), "the operand row of the neighbouring channel")
    # padding column M read as a value of the rms (against the frame behind the last one; the signal's last value past its end)
    xe = torch.cat([x.double(), x.double()[:, :, -1:].expand(-1, -1, S)], 2)
    ae = torch.cat([a64, torch.full((N, C, 1), rms(a64), dtype=F64)], 2)
    fl(wgrad_ref(ae, xe, K_, S), "padding column M read as a value of the rms")
    if split is not None and split["msplit"] > 1:
        a2 = a64.clone()
        a2[:, :, :split["mchunk"]] *= 2
        fl(wgrad_ref(a2, x, K_, S), "one split chunk added twice")
    if lo_term is not None:
        fl(ref - lo_term, "min_a of the coded operand dropped")


def wg_body(case, mode):
    """fqss_frames_wgrad1 / _q on the matrix cores and the fallback fqss_frames_wgrad (aligned and misaligned operand rows) on the same
    operands, into a non-zero gw.  "int": the integer sums bit for bit; "real": each against float64, fqss_frames_wgrad1 against
    fqss_frames_wgrad within the sum of their bounds"""
    k = WG_CASES.index(case)
    N, C, M, K_, S, tail = case
    a, c, x, start = wg_operands(case, mode, 3000 + k)
    lo, hi = (ILO, ILO + 255.0) if mode == "int" else (LO, HI)
    tag0 = f"wgrad {mode} {case}"
    fails = []
    ref = wgrad_ref(a, x, K_, S)
    refq = wgrad_ref(dec(c, lo, hi), x, K_, S)
    if mode == "int":
        assert float(delta32(lo, hi)) == 1.0
        assert exact_ok(wgrad_ref(a.abs(), x.abs(), K_, S) + start.abs(), wgrad_ref(dec(c, lo, hi).abs(), x.abs(), K_, S) + start.abs()), tag0
        st, stq = start, start
    else:
        st, stq = real_start(ref, k), real_start(refq, 50 + k)
    fr = frames(x, K_, S, M)
    r32 = torch.einsum("ncm,nimk->cik", a, fr)
    runs = [("fqss_frames_wgrad1", "al", "wg1"), ("fqss_frames_wgrad", "al", "wgfb"), ("fqss_frames_wgrad", "odd" if k % 2 else "off", "wgfb")]
    got = {}
    for entry, kind, fam in runs:
        if not have(entry):
            continue
        g_ = wg_run(entry, a, x, st, K_, S, kind)
        tag = f"{tag0} {entry} {kind}"
        if mode == "int":
            assert torch.equal(g_, (ref + st.double()).float()), (tag, int((g_ != (ref + st.double()).float()).sum()))
        else:
            measure(fam, "gw", g_.double() - st.double(), ref, r32, tag, fails)
        got[(entry, kind)] = g_
        if kind == "al":
            wg_mutations(fam, a.double(), x, K_, S, ref, tag, fails, mode, split=wgrad1_dispatch(N, C, M, False) if fam == "wg1" else None)
    if mode == "real" and len(got) > 1:
        d = errs(got[("fqss_frames_wgrad1", "al")].double() - st.double(), got[("fqss_frames_wgrad", "al")].double() - st.double())
        print(f"PAIR wgrad1 vs fallback e_elem {d[0]:.2e} | {tag0}")
        if not d[0] <= BOUND["wg1"]["gw"][0] + BOUND["wgfb"]["gw"][0]:
            fails.append((tag0, "pair", d))
    if have("fqss_frames_wgrad1_q"):
        g_ = wg_run("fqss_frames_wgrad1_q", c, x, stq, K_, S, "al", lo=lo, hi=hi)
        tag = f"{tag0} fqss_frames_wgrad1_q"
        if mode == "int":
            assert torch.equal(g_, (refq + stq.double()).float()), (tag, int((g_ != (refq + stq.double()).float()).sum()))
        else:
            measure("wg1q", "gw", g_.double() - stq.double(), refq, torch.einsum("ncm,nimk->cik", dec32(c, lo, hi), fr), tag, fails)
        lo_term = f32(lo).double() * fr.double().sum((0, 2))[None].expand(C, -1, -1)
        wg_mutations("wg1q", dec(c, lo, hi), x, K_, S, refq, tag, fails, mode, split=wgrad1_dispatch(N, C, M, True), lo_term=lo_term)
    assert not fails, fails


def wg1s_body(case, mode):
    """fqss_frames_wgrad1s on channel ci of a Ci = 2 signal against column block ci of fqss_frames_wgrad (and float64 / the integers)"""
    k = WG_CASES.index(case)
    N, C, M, K_, S, tail = case
    a, _, x, start = wg_operands(case, mode, 3500 + k, Ci=2)
    ref = wgrad_ref(a, x, K_, S)
    tag0 = f"wgrad1s {mode} {case}"
    fails = []
    if mode == "int":
        assert exact_ok(wgrad_ref(a.abs(), x.abs(), K_, S) + start.abs()), tag0
        st = start
    else:
        st = real_start(ref, 70 + k)
    r32 = torch.einsum("ncm,nimk->cik", a, frames(x, K_, S, M))
    fb = wg_run("fqss_frames_wgrad", a, x, st, K_, S, "al")
    if mode == "int":
        assert torch.equal(fb, (ref + st.double()).float()), tag0
    else:
        measure("wgfb", "gw", fb.double() - st.double(), ref, r32, f"{tag0} fqss_frames_wgrad Ci=2", fails)
    for ci in (0, 1):
        g_ = wg_run("fqss_frames_wgrad1s", a, x, st, K_, S, "al", ci=ci)
        if mode == "int":
            assert torch.equal(g_[:, ci], (ref + st.double()).float()[:, ci]), (tag0, ci)
        else:
            measure("wg1", "gw", g_[:, ci].double() - st[:, ci].double(), ref[:, ci], r32[:, ci], f"{tag0} ci={ci}", fails)
            d = errs(g_[:, ci].double() - st[:, ci].double(), fb[:, ci].double() - st[:, ci].double())
            if not d[0] <= BOUND["wg1"]["gw"][0] + BOUND["wgfb"]["gw"][0]:
                fails.append((tag0, ci, "pair", d))
        floor_or_diff = wgrad_ref(a, x.flip(1), K_, S)[:, ci]
        if mode == "int":
            differs(floor_or_diff, ref[:, ci], "the other channel's signal", tag0)
        else:
            floor("wg1", "gw", floor_or_diff, ref[:, ci], "the other channel's signal", tag0, fails)
    assert not fails, fails


@gpu
@pytest.mark.parametrize("case", WG_CASES, ids=str)
def test_frames_wgrad_exact_integers(case):
    """the four weight-gradient entries on integers into an integer gw: every term exactly once through the fp32 atomics, the LDS
    cross-wave sums and the split partial sums"""
    wg_body(case, "int")
    if WG_CASES.index(case) % 2 == 0:
        wg1s_body(case, "int")


@gpu
@pytest.mark.parametrize("case", WG_CASES, ids=str)
def test_frames_wgrad_against_fp64(case):
    """heavy-tailed operand, a waveform with a DC offset, gw from non-zero random values: within the family bounds of float64"""
    wg_body(case, "real")
    if WG_CASES.index(case) % 2 == 1 or WG_CASES.index(case) >= 10:
        wg1s_body(case, "real")


def wg21_body(case, mode):
    k = WG21_CASES.index(case)
    N, C, M, K_, S, tail = case
    fails = []
    for Ci in (1, 2):
        a, _, x, start = wg_operands(case, mode, 3800 + 2 * k + Ci, Ci=Ci)
        ref = wgrad_ref(a, x, K_, S)
        st = start if mode == "int" else real_start(ref, 90 + k)
        for kind in ("al", "odd"):
            g_ = wg_run("fqss_frames_wgrad", a, x, st, K_, S, kind)
            tag = f"wgrad (2, 1) {mode} {case} Ci={Ci} {kind}"
            if mode == "int":
                assert exact_ok(wgrad_ref(a.abs(), x.abs(), K_, S) + st.abs()) and torch.equal(g_, (ref + st.double()).float()), tag
            else:
                measure("wgfb", "gw", g_.double() - st.double(), ref, torch.einsum("ncm,nimk->cik", a, frames(x, K_, S, M)), tag, fails)
        wg_mutations("wgfb", a.double(), x, K_, S, ref, f"wgrad (2, 1) {case} Ci={Ci}", fails, mode)
    assert not fails, fails


@gpu
@pytest.mark.parametrize("case", WG21_CASES, ids=str)
def test_frames_wgrad_generic_window(case):
    """fqss_frames_wgrad at (K, S) = (2, 1), Ci in {1, 2}: exact integers and float64"""
    wg21_body(case, "int")
    wg21_body(case, "real")


@gpu
def test_frames_wgrad_refusals():
    """every FQSS_REQUIRE / set_error of the four entries; misaligned rows of the _wgrad1 trio return FQSS_EINVAL and leave gw
    untouched (callers fall back to fqss_frames_wgrad); N = 0 and M = 0 are no-ops"""
    N, C, M, K_, S = 2, 3, 5, 16, 8
    T = (M - 1) * S + K_
    g = gen(9)
    a, x, st = torch.randn(N, C, M, generator=g), torch.randn(N, 1, T, generator=g), torch.randn(C, 1, K_, generator=g)
    c = codes(g, N, C, M)
    ab, cb, xb = Blk(N * C, M, 8, fill=a), Cod(N * C, M, 16, fill=c), Blk(N, T, T, fill=x)
    gw = Blk(C, K_, K_, fill=st)
    lo, hi = sc(0.0), sc(1.0)
    St = stream()

    def fb(a_=ab.ptr, x_=xb.ptr, g_=gw.ptr, N=N, C=C, Ci=1, M=M, ld=8, T=T, K_=K_, S=S):
        refused("fqss_frames_wgrad", a_, x_, g_, N, C, Ci, M, ld, T, K_, S, St)

    def w1(a_=True, x_=xb.ptr, g_=gw.ptr, N=N, C=C, M=M, ld=None, T=T, K_=K_, S=S):
        refused("fqss_frames_wgrad1", ab.ptr if a_ else None, x_, g_, N, C, M, ld or 8, T, K_, S, St)
        refused("fqss_frames_wgrad1s", ab.ptr if a_ else None, x_, T, g_, K_, N, C, M, ld or 8, T, K_, S, St)
        refused("fqss_frames_wgrad1_q", cb.ptr if a_ else None, lo.ptr, hi.ptr, x_, g_, N, C, M, ld or 16, T, K_, S, St)

    for kw in (dict(a_=None), dict(x_=None), dict(g_=None), dict(N=-1), dict(C=0), dict(Ci=0), dict(M=-1), dict(ld=4), dict(K_=0), dict(S=0),
               dict(T=T - 1)):
        fb(**kw)
    for kw in (dict(a_=False), dict(x_=None), dict(g_=None), dict(N=-1), dict(C=0), dict(M=-1), dict(ld=4), dict(K_=0), dict(S=0), dict(T=T - 1),
               dict(K_=8, S=4), dict(K_=2, S=1), dict(N=65536)):
        w1(**kw)
    refused("fqss_frames_wgrad1_q", cb.ptr, None, hi.ptr, xb.ptr, gw.ptr, N, C, M, 16, T, K_, S, St)
    refused("fqss_frames_wgrad1_q", cb.ptr, lo.ptr, None, xb.ptr, gw.ptr, N, C, M, 16, T, K_, S, St)
    refused("fqss_frames_wgrad1s", ab.ptr, xb.ptr, T - 1, gw.ptr, K_, N, C, M, 8, T, K_, S, St)            # sig_ns < T
    refused("fqss_frames_wgrad1s", ab.ptr, xb.ptr, T, gw.ptr, K_ - 1, N, C, M, 8, T, K_, S, St)            # ld_gw < K
    assert gw.unchanged()
    # misaligned rows: FQSS_EINVAL, gw untouched (wg_run asserts both)
    for kind in ("odd", "off"):
        wg_run("fqss_frames_wgrad1", a, x, st, K_, S, kind, expect=EINVAL)
        wg_run("fqss_frames_wgrad1s", a, x, st, K_, S, kind, ci=0, expect=EINVAL)
        wg_run("fqss_frames_wgrad1_q", c, x, st, K_, S, kind, lo=0.0, hi=1.0, expect=EINVAL)
    for n_, m_ in ((0, M), (N, 0)):
        call("fqss_frames_wgrad", ab.ptr, xb.ptr, gw.ptr, n_, C, 1, m_, 8, T, K_, S, St)
        call("fqss_frames_wgrad1", ab.ptr, xb.ptr, gw.ptr, n_, C, m_, 8, T, K_, S, St)
        call("fqss_frames_wgrad1s", ab.ptr, xb.ptr, T, gw.ptr, K_, n_, C, m_, 8, T, K_, S, St)
        call("fqss_frames_wgrad1_q", cb.ptr, lo.ptr, hi.ptr, xb.ptr, gw.ptr, n_, C, m_, 16, T, K_, S, St)
    assert gw.unchanged()
    all_unchanged(a=ab, c=cb, x=xb)


# ============================================================================================================ 5. deterministic mode
@pytest.fixture
def det_off():
    yield
    if K is not None:
        K.DetMode.off()          # (the control block is device-wide: no later test may run under it)


@gpu
def test_frames_wgrad_deterministic_mode(det_off):
    """FQSS_DETERMINISTIC=1: the split shapes of the four entries into slices of an attached arena, twice -- bit-identical after
    fqss_det_finish, within the family bound of float64, the integer slots exact, nothing beside the slots"""
    shapes = [(1, 8, 2100, 32, 16, 0), (3, 130, 513, 16, 8, 0), (1, 8, 4200, 16, 8, 4)]
    g = gen(77)
    jobs, off = [], 64          # (name, entry, operands, offset, reference [C][Ci][K], family, start, exact)
    for k, case in enumerate(shapes):
        N, C, M, K_, S, tail = case
        for mode in ("real", "int"):
            a, c, x, start = wg_operands(case, mode, 4000 + k)
            a2, _, x2, start2 = wg_operands(case, mode, 4100 + k, Ci=2)
            lo, hi = (ILO, ILO + 255.0) if mode == "int" else (LO, HI)
            for name, entry, aa, xx, fam in ((f"w1 {case} {mode}", "fqss_frames_wgrad1", a, x, "wg1"), (f"fb {case} {mode}", "fqss_frames_wgrad", a2, x2, "wgfb"),
                                             (f"w1s {case} {mode}", "fqss_frames_wgrad1s", a2, x2, "wg1"), (f"q {case} {mode}", "fqss_frames_wgrad1_q", c, x, "wg1q")):
                ref = wgrad_ref(dec(aa, lo, hi) if entry.endswith("_q") else aa, xx, K_, S)
                st = ints(g, 1000, *ref.shape) if mode == "int" else real_start(ref, 4200 + len(jobs))
                if mode == "int":
                    assert exact_ok(wgrad_ref((dec(aa, lo, hi) if entry.endswith("_q") else aa).abs(), xx.abs(), K_, S) + st.abs())
                coded = entry.endswith("_q")
                ld, _ = xlay(M, "al", coded=coded, extra=8)
                ab = (Cod if coded else Blk)(N * C, M, ld, fill=aa)
                xb = Blk(xx.shape[0] * xx.shape[1], xx.shape[2], xx.shape[2], fill=xx)
                jobs.append(dict(name=name, entry=entry, a=ab, x=xb, off=off, ref=ref, fam=fam, st=st, exact=mode == "int", case=case, lo=sc(lo), hi=sc(hi),
                                 Ci=xx.shape[1]))
                off += (ref.numel() + 63) // 64 * 64 + 64
    arena = torch.zeros(off, device=L.DEV)
    det = K.DetMode()
    det.attach(0, arena)
    det.activate()
    runs = []
    St = stream()
    for _ in range(2):
        arena.zero_()
        for j in jobs:
            arena[j["off"]:j["off"] + j["ref"].numel()].copy_(j["st"].reshape(-1))
        for j in jobs:
            N, C, M, K_, S, tail = j["case"]
            T, p, ab, xb = j["x"].M, arena.data_ptr() + 4 * j["off"], j["a"], j["x"]
            if j["entry"] == "fqss_frames_wgrad":
                call(j["entry"], ab.ptr, xb.ptr, p, N, C, 2, M, ab.ld, T, K_, S, St)
            elif j["entry"] == "fqss_frames_wgrad1":
                call(j["entry"], ab.ptr, xb.ptr, p, N, C, M, ab.ld, T, K_, S, St)
            elif j["entry"] == "fqss_frames_wgrad1s":
                for ci in (0, 1):
                    call(j["entry"], ab.ptr, xb.ptr + 4 * ci * T, 2 * T, p + 4 * ci * K_, 2 * K_, N, C, M, ab.ld, T, K_, S, St)
            else:
                call(j["entry"], ab.ptr, j["lo"].ptr, j["hi"].ptr, xb.ptr, p, N, C, M, ab.ld, T, K_, S, St)
        det.finish(0)
        sync()
        runs.append(arena.cpu().clone())
    K.DetMode.off()
    for j in jobs:
        all_unchanged(a=j["a"], x=j["x"])
    assert torch.equal(runs[0], runs[1]), "deterministic mode: the sums of two runs differ"
    r, beside, fails = runs[0], torch.ones(off, dtype=torch.bool), []
    for j in jobs:
        o, ref = j["off"], j["ref"]
        beside[o:o + ref.numel()] = False
        got = r[o:o + ref.numel()].reshape(ref.shape)
        if j["exact"]:
            assert torch.equal(got, (ref + j["st"].double()).float()), (j["name"], "exact in deterministic mode")
        else:
            measure(j["fam"], "gw", got.double() - j["st"].double(), ref, None, f"deterministic {j['name']}", fails)
    assert bool((r[beside] == 0).all()), "a write beside the gradient slots"
    assert not fails, fails


# ===================================================================================================================== 6. the mirror
def test_dispatch_of_the_named_shapes():
    """conv_dispatch / ola_dispatch / wgrad1_dispatch give the values the docstring's table names (no GPU)"""
    check_named_dispatch()
