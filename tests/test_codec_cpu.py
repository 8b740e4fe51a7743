"""The CPU side of tests/test_gpu_codec_kernels.py.  No GPU.
  - the float64 references of that file against float64 F.conv1d, F.conv_transpose1d and their autograd; the splitter emulations against
    the reference-generated fixture tests/golden/codec_split.npz (tools/make_goldens_codec.py: process.preprocess in both forms and row by
    row) and oracle.fqss_oracle.split / oracle.htdemucs_oracle.split_raw;
  - the mirror of the launch code on the shapes the docstring's table names, and that every value of every axis the issue names is in the
    grids;
  - the case bodies of the GPU file on the CPU backend (fqss_amd/csrc/cpu/libfqss_cpu.so through `_lib.set_backend("cpu")`) for the
    entries it has -- fqss_splitter2, _rows, fqss_frames_conv_fwd, fqss_ola_convtr_fwd, fqss_frames_wgrad, _wgrad1, _wgrad1s -- in the
    same NaN-padded, guarded buffers: the harness, the case builders and the exactness conditions are proven before anything reaches a
    GPU, and the CPU backend's own bounds handling is under the same guards."""
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle.fqss_oracle as O
import oracle.htdemucs_oracle as OH
import tests.test_gpu_codec_kernels as C
import tests.test_gpu_layout_spectral_kernels as L
import tests.test_gpu_qgemm_kernels as Q
from tests.test_gpu_layout_spectral_kernels import F64, errs


def _aligned_full(real):
    """torch.full for flat host buffers, 256-B aligned as the device allocator's are (Blk / Cod assert it; the dispatch reads it)"""

    def full(size, fill_value, **kw):
        n = int(np.prod(size))
        if len(size) != 1 or str(kw.get("device", "cpu")) != "cpu":
            return real(size, fill_value, **kw)
        es = torch.empty(0, dtype=kw.get("dtype", torch.float32)).element_size()
        raw = np.empty(n * es + 256, dtype=np.uint8)
        shift = -raw.ctypes.data % 256
        # (a storage of its own that begins at the aligned address: Blk / Cod address their views by storage offset)
        return torch.from_numpy(raw[shift:shift + n * es]).view(kw.get("dtype", torch.float32)).fill_(fill_value)

    return full


@pytest.fixture()
def cpu_backend(monkeypatch):
    """the GPU file's buffers on the host, its calls on libfqss_cpu.so"""
    from fqss_amd import _lib
    if not os.path.exists(_lib.CPU_SO_PATH):
        subprocess.check_call(["make", "-C", os.path.dirname(_lib.CPU_SO_PATH)])
    _lib.set_backend("cpu")
    monkeypatch.setattr(L, "DEV", "cpu")
    monkeypatch.setattr(Q, "DEV", "cpu")
    monkeypatch.setattr(torch, "full", _aligned_full(torch.full))
    monkeypatch.setattr(C, "_lib", _lib)
    yield
    _lib.set_backend("hip")


def test_references_on_cpu(golden):
    g = Q.gen(1)
    N, Ci, Co, M, K_, S, tail = 3, 2, 5, 9, 16, 8, 5
    T = (M - 1) * S + K_ + tail
    x, w = torch.randn(N, Ci, T, generator=g).double().requires_grad_(), torch.randn(Co, Ci, K_, generator=g).double().requires_grad_()
    add = torch.randn(N, Co, M, generator=g)
    z = F.conv1d(x, w, stride=S)[:, :, :M]
    assert errs(z.detach(), C.conv_ref(x.detach(), w.detach(), S, M))[0] <= 1e-13
    assert errs(z.detach() + add.double(), C.conv_ref(x.detach(), w.detach(), S, M, add))[0] <= 1e-13
    assert bool((C.conv_mag(x.detach(), w.detach(), S, M, add) >= C.conv_ref(x.detach(), w.detach(), S, M, add).abs() * (1 - 1e-12)).all())
    # the weight gradient of the framing conv is its autograd; the decoder is the conv's input gradient on a signal without a tail
    a = Q.heavy(g, N, Co, M).double()
    z.backward(a)
    assert errs(w.grad, C.wgrad_ref(a, x.detach(), K_, S))[0] <= 1e-13
    gx = x.grad[:, :, :(M - 1) * S + K_]
    for ci in range(Ci):
        assert errs(gx[:, ci], C.ola_ref(a, w.detach()[:, ci], S))[0] <= 1e-13
    assert float(x.grad[:, :, (M - 1) * S + K_:].abs().max()) == 0.0
    for K2, S2 in ((16, 8), (32, 16), (2, 1)):
        xd, wd = torch.randn(2, 7, 11, generator=g).double(), torch.randn(7, K2, generator=g).double()
        assert errs(F.conv_transpose1d(xd, wd[:, None, :], stride=S2)[:, 0], C.ola_ref(xd, wd, S2))[0] <= 1e-13
    # the coded operand: delta c + lo with the fp32 step
    c = Q.codes(g, 2, 3, 5)
    assert torch.equal(C.dec(c, C.ILO, C.ILO + 255.0), c.double() + C.ILO) and float(Q.delta32(C.ILO, C.ILO + 255.0)) == 1.0
    assert errs(C.dec32(c, C.LO, C.HI), C.dec(c, C.LO, C.HI))[0] <= 2e-7
    # the splitter emulations against the reference's process.preprocess
    gs = golden("codec_split")
    xs = torch.from_numpy(gs["x"])
    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(O.split(xs, 2)), bits(torch.from_numpy(gs["norm"])))
    assert torch.equal(bits(C.split_raw_emul(xs)), bits(torch.from_numpy(gs["raw"])))
    assert torch.equal(bits(OH.split_raw(xs.unsqueeze(1))), bits(torch.from_numpy(gs["raw"])))
    assert torch.equal(bits(C.split_rows_emul(xs)), bits(torch.from_numpy(gs["rows"])))
    assert not torch.equal(torch.from_numpy(gs["rows"]), torch.from_numpy(gs["norm"]))
    sil = C.split_rows_emul(torch.zeros(1, 8))
    assert bool(torch.isnan(sil).all()), "a silent row is NaN in the reference (0 / 0 through torch.clip)"
    # the edge inputs are what they claim: values on bin edges, +-thr, +-0, denormals
    xe = C.split_inputs(3, 255, 11)
    thr = float(xe.abs().max())
    assert float(xe.view(-1)[0]) == thr and float(xe.view(-1)[1]) == -thr and 0 < float(xe.view(-1)[4]) < 1.2e-38
    n = O.split(xe, 2)
    assert float(n[:, 0].max()) == 127 / 128 and float(n[:, 0].min()) == -1.0
    assert bool(torch.signbit(xe.view(-1)[3])) and float(xe.view(-1)[3]) == 0.0


def test_dispatch_mirror_and_grids():
    C.check_named_dispatch()
    ax = lambda cases, k: {c[k] for c in cases}
    assert set(C.CONV_NAMED) <= {c[:6] for c in C.CONV_CASES}
    assert ax(C.CONV_CASES, 2) >= {1, 3, 5} and ax(C.CONV_CASES, 3) >= {1, 3, 4, 5, 255, 256, 257}
    assert {(c[1], c[4], c[5]) for c in C.CONV_CASES} >= {(1, 2, 1), (2, 2, 1), (1, 16, 8), (2, 16, 8), (1, 32, 16), (2, 32, 16)}
    assert any(c[6] for c in C.CONV_CASES)
    assert ax(C.DEC_CASES, 1) == {1, 3, 4, 5, 16, 17, 20, 33, 130} and ax(C.DEC_CASES, 0) == {1, 3}
    assert {c[2] for c in C.DEC_CASES if c[3:] == (16, 8)} == {1, 2, 3, 4, 59, 60, 61, 119, 120, 121}
    assert {c[2] for c in C.DEC_CASES if c[3:] == (32, 16)} == {c[2] for c in C.DEC_CASES if c[3:] == (2, 1)} == {62, 63, 64}
    assert ax(C.WG_CASES, 1) >= {1, 15, 16, 17, 63, 64, 65, 130} and ax(C.WG_CASES, 2) >= {1, 7, 8, 9, 127, 128, 129, 255, 256, 257}
    assert {c[:3] for c in C.WG_CASES} >= set(C.WG_NAMED) and {c[3:5] for c in C.WG_CASES} == {(16, 8), (32, 16)}
    assert any(c[5] for c in C.WG_CASES) and {c[3:5] for c in C.WG21_CASES} == {(2, 1)}
    # the second pass of the frame loop and the split are reached by the named shapes
    d = [C.wgrad1_dispatch(*c[:3], False) for c in C.WG_CASES]
    assert max(x["passes"] for x in d) >= 3 and max(x["msplit"] for x in d) >= 9
    # every conv case with a second LDS tap tile or a ragged last slice
    dc = [C.conv_dispatch(*c[:6], (c[3] - 1) * c[5] + c[4] + c[6]) for c in C.CONV_CASES]
    assert sum(x.get("tiles", 1) > 1 for x in dc) == 3 and any(x.get("zs", 1) > 1 and x["last"] % 32 for x in dc)
    assert sum(x["form"] == "generic" for x in dc) == 2


def test_splitter_on_the_cpu_backend(cpu_backend):
    C.splitter_body(C.SPLIT_SHAPES[:3] + [(2, 5000)])
    C.splitter_rows_body(long_row=False)


@pytest.mark.parametrize("case", [c for c in C.CONV_CASES if c[0] * c[2] * c[3] <= 500000], ids=str)
def test_frames_conv_on_the_cpu_backend(cpu_backend, case):
    C.conv_body(case, "int")
    C.conv_body(case, "real")


@pytest.mark.parametrize("case", C.DEC_CASES, ids=str)
def test_decoder_on_the_cpu_backend(cpu_backend, case):
    C.dec_body(case, "int", modes=(0,))
    C.dec_body(case, "real", modes=(0,))


@pytest.mark.parametrize("case", C.WG_CASES + C.WG21_CASES, ids=str)
def test_frames_wgrad_on_the_cpu_backend(cpu_backend, case):
    if case in C.WG21_CASES:
        C.wg21_body(case, "int")
        C.wg21_body(case, "real")
        return
    C.wg_body(case, "int")
    C.wg_body(case, "real")
    C.wg1s_body(case, "int")
    C.wg1s_body(case, "real")
