"""The batched chunked-inference path without a GPU: fqss_splitter2_rows, fqss_chunk_gather, fqss_sisnr_chunks and
fqss_infer_ola_chunks on the CPU backend (fqss_amd/csrc/cpu/libfqss_cpu.so, `_lib.set_backend("cpu")`) against NumPy, and
`process.model_infer(chunk_batch=G)` against the oracle's chunk-by-chunk loop.

Tolerances.  SI-SNR: rtol 1e-5, atol 1e-4 dB, the bounds of test_gpu_infer.test_sisnr_matrix_and_swap (fp64 moments against an fp64
two-pass checker; the value is stored as fp32).  Maps are compared exactly, on inputs whose best and second-best SI-SNR differ by at
least 3 dB in every chunk (asserted).  Overlap-add: 1e-6 * max|chunk| absolute -- a sample is the weighted mean of at most
1 / (1 - overlap) chunk samples (10 at overlap 0.9), every term carries one fp32 rounding of 2^-24 relative, then one division."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import helpers_infer_batched as H


@pytest.fixture()
def cpu_backend():
    from fqss_amd import _lib
    if not os.path.exists(_lib.CPU_SO_PATH):
        subprocess.check_call(["make", "-C", os.path.dirname(_lib.CPU_SO_PATH)])
    _lib.set_backend("cpu")
    yield
    _lib.set_backend("hip")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_splitter2_rows_equals_splitter2_row_by_row(cpu_backend):
    from fqss_amd import kernels as K
    x = torch.randn(4, 257, generator=torch.Generator().manual_seed(0)) * 0.3
    x = x * torch.tensor([1.0, 0.1, 1e-3, 7.0])[:, None]
    got = K.splitter2_rows(x)
    want = torch.cat([K.splitter2(x[b:b + 1]) for b in range(4)])
    assert got.shape == (4, 2, 257) and torch.equal(got, want)
    assert not torch.equal(got, K.splitter2(x))                      # the global threshold is another function
    assert torch.equal(K.splitter2_rows(x.unsqueeze(1)), want)       # [B, 1, T]
    # a silent row divides by a zero threshold in its own row only, and comes out as a silent chunk does chunk by chunk (bit images
    # compared, so that NaN would count as equal to NaN)
    x[2] = 0.0
    got = K.splitter2_rows(x)
    assert torch.equal(got[2:3].view(torch.int32), K.splitter2(x[2:3]).view(torch.int32))
    assert torch.equal(got[[0, 1, 3]], want[[0, 1, 3]])


@pytest.mark.parametrize("L,seg,overlap", H.GEOMETRIES)
def test_chunk_gather_equals_slicing(cpu_backend, L, seg, overlap):
    from fqss_amd import kernels as K
    stride, N, _ = H.geometry(L, seg, overlap)
    mix = np.random.RandomState(1).randn(1, L).astype(np.float32)
    for G in (1, 2, N, N + 3):                                       # N + 3 and the last group of 2 run past the last chunk
        for k0 in range(0, N, G):
            got = K.chunk_gather(T(mix), seg, stride, k0, G)
            assert got.shape == (G, 1, seg) and np.array_equal(got.numpy(), H.gather_ref(mix, seg, stride, k0, G)), (G, k0)


@pytest.mark.parametrize("S", [2, 3])
def test_sisnr_chunks_against_fp64(cpu_backend, S):
    from fqss_amd import kernels as K
    L, seg, overlap = 3100, 1000, 0.25                               # 5 chunks, the last 100 samples long
    stride, N, _ = H.geometry(L, seg, overlap)
    ref, est = H.sisnr_case(L, seg, overlap, S, seed=2)
    db64, mp64, margin = H.sisnr_chunks_ref(est, ref, seg, stride)
    assert margin >= H.MARGIN_DB, margin
    assert mp64[1].tolist() == [[S - 1 - d, 1 if S - 1 - d == d else -1] for d in range(S)]      # a swap ...
    assert mp64[2, 0].tolist() == [S - 1, -1]                        # ... and a contested target: the last claimant keeps it
    pitched = torch.full((S, L + 5), float("nan"))
    pitched[:, :L] = T(ref)
    for G in (2, 5, 8):
        n_pad = -(-N // G) * G
        e = torch.full((n_pad, S, seg), float("nan"))
        e[:N] = T(est)
        db, mp = torch.empty(n_pad, S, S), torch.zeros(n_pad, S, 2, dtype=torch.int32)
        for k0 in range(0, N, G):
            K.sisnr_chunks(e[k0:k0 + G], pitched[:, :L], stride, k0, db=db[k0:k0 + G], mp=mp[k0:k0 + G])
        np.testing.assert_allclose(db[:N].numpy(), db64, rtol=1e-5, atol=1e-4)
        assert np.array_equal(mp[:N].numpy(), mp64)


@pytest.mark.parametrize("L,seg,overlap", H.GEOMETRIES + [(3100, 1000, 0.9)])
def test_infer_ola_chunks_against_fp64(cpu_backend, L, seg, overlap):
    from fqss_amd import kernels as K
    stride, N, _ = H.geometry(L, seg, overlap)
    for S, C in ((2, 1), (3, 2)):
        chunks, maps = H.ola_case(L, seg, overlap, S, C, seed=3, pad_chunks=2)
        tol = 1e-6 * float(np.nanmax(np.abs(chunks)))
        for mp in (maps, None):
            got = K.infer_ola_chunks(T(chunks), None if mp is None else T(mp), L, stride)
            err = np.abs(got.numpy() - H.ola_ref(chunks, mp, L, stride)).max()
            print(f"L {L} seg {seg} overlap {overlap} S {S} C {C} maps {mp is not None}: max err {err:.3g} (bound {tol:.3g})")
            assert got.shape == (S, C, L) and err <= tol
        got3 = K.infer_ola_chunks(T(chunks[:, :, 0]), T(maps), L, stride)                        # [N, S, seg] -> [S, L]
        assert got3.shape == (S, L) and torch.equal(got3, K.infer_ola_chunks(T(chunks[:, :, :1]), T(maps), L, stride)[:, 0])


# ---- end to end against the oracle's chunk-by-chunk loop
FIR = torch.tensor([[0.5, 0.5, 0.0], [0.25, -0.5, 0.25]])          # a low-pass and a high-pass: two clearly different "sources"


def per_item_fwd(x):
    """[B, 1, T] -> [B, 2, T]: a fixed two-source FIR whose gain depends on the item's own maximum, as the per-chunk normalisation of
    the real models does; shifts, products and sums only, so every item is computed alike whatever the batch"""
    x = x.reshape(x.shape[0], -1)
    gain = 1.0 / (0.05 + x.abs().amax(dim=1, keepdim=True))
    xp = torch.nn.functional.pad(x, (2, 0))
    out = [(h[0] * xp[:, 2:] + h[1] * xp[:, 1:-1] + h[2] * xp[:, :-2]) * gain for h in FIR]
    return torch.stack(out, dim=1)


@pytest.mark.parametrize("G", [1, 2, 5, 8])
def test_model_infer_chunk_batch_matches_the_oracle(cpu_backend, G):
    import oracle.fqss_oracle as O
    from fqss_amd.process import model_infer
    L, seg, overlap = 3100, 1000, 0.25
    mix = torch.randn(1, L, generator=torch.Generator().manual_seed(4)) * 0.2
    mix[:, L // 2:] *= 0.1                                           # a global gain would differ from the per-item one
    whole = per_item_fwd(mix.unsqueeze(0))[0]
    target = torch.stack([whole[1], -whole[0]])                      # every chunk moves both sources (and flips their sign)
    calls = []

    def fwd(x):
        calls.append(tuple(x.shape))
        return per_item_fwd(x)

    for tgt in (target, None):
        want = O.model_infer(per_item_fwd, mix, 2, segment=seg, overlap=overlap, target=tgt)
        del calls[:]
        got = model_infer(fwd, mix, n_srcs=2, segment=seg, overlap=overlap, device="cpu", target=tgt, chunk_batch=G)
        assert calls == [(G, 1, seg)] * -(-5 // G)                   # one model shape, ceil(N / G) forwards
        tol = 1e-6 * float(per_item_fwd(torch.from_numpy(H.gather_ref(mix.numpy(), seg, 750, 0, 5))).abs().max())
        err = float((got - want).abs().max())
        print(f"G {G} target {tgt is not None}: max err {err:.3g} (bound {tol:.3g})")
        assert got.shape == want.shape == (2, L) and err <= tol
    # with the target the estimates come back in the target's order and sign
    got = model_infer(fwd, mix, n_srcs=2, segment=seg, overlap=overlap, device="cpu", target=target, chunk_batch=G)
    plain = model_infer(fwd, mix, n_srcs=2, segment=seg, overlap=overlap, device="cpu", chunk_batch=G)
    assert torch.equal(got[0], -plain[1]) and torch.equal(got[1], -plain[0])


def test_refusals(cpu_backend):
    from fqss_amd import _lib, ops, process
    from fqss_amd import kernels as K
    mix = torch.randn(1, 3100)
    for G in (0, -2):
        with pytest.raises(ValueError, match="chunk_batch"):
            process.model_infer(per_item_fwd, mix, n_srcs=2, segment=1000, device="cpu", chunk_batch=G)
    with pytest.raises(ValueError, match="hop"):
        process.model_infer(per_item_fwd, mix, n_srcs=2, segment=1000, overlap=1.0, device="cpu", chunk_batch=2)
    with pytest.raises(NotImplementedError, match="one-channel"):
        process.model_infer(per_item_fwd, torch.randn(2, 3100), n_srcs=2, segment=1000, device="cpu", chunk_batch=2)
    # the per-item switch: one-channel waveforms only, off outside the block, the plain input untouched
    x3 = torch.randn(2, 2, 300)
    with ops.split_per_item(True):
        assert ops.SPLIT_PER_ITEM
        for kw in (dict(), dict(normalize=False)):
            with pytest.raises(NotImplementedError, match="split_per_item"):
                process.preprocess(x3, n_splitter=2, **kw)
        assert process.preprocess(x3, n_splitter=1) is x3
        rows = torch.randn(3, 1, 300) * torch.tensor([1.0, 0.1, 3.0])[:, None, None]
        assert torch.equal(process.preprocess(rows, n_splitter=2), K.splitter2_rows(rows))
    assert not ops.SPLIT_PER_ITEM and torch.equal(process.preprocess(rows, n_splitter=2), K.splitter2(rows))
    # the C ABI: null pointers and bad shapes are refused before anything is written
    f = torch.zeros(4096)
    i = torch.zeros(64, dtype=torch.int32)
    p, q = f.data_ptr(), i.data_ptr()
    bad = [("fqss_chunk_gather", (None, p, 3100, 1000, 750, 0, 2, None)),
           ("fqss_chunk_gather", (p, p, 3100, 1000, 750, 5, 2, None)),           # k0 past the last chunk
           ("fqss_chunk_gather", (p, p, 3100, 1000, 1001, 0, 2, None)),          # hop > segment
           ("fqss_chunk_gather", (p, p, 3100, 1000, 0, 0, 2, None)),
           ("fqss_chunk_gather", (p, p, 3100, 1000, 750, 0, 0, None)),
           ("fqss_splitter2_rows", (p, p, 2, 100, None, None)),
           ("fqss_splitter2_rows", (p, p, 0, 100, q, None)),
           ("fqss_sisnr_chunks", (p, p, p, None, 2, 2, 100, 75, 0, 310, 310, None)),
           ("fqss_sisnr_chunks", (p, p, p, q, 2, 17, 100, 75, 0, 310, 310, None)),   # S > 16
           ("fqss_sisnr_chunks", (p, p, p, q, 2, 2, 100, 75, 0, 310, 309, None)),    # ld_r < L
           ("fqss_sisnr_chunks", (p, p, p, q, 2, 2, 100, 75, 5, 310, 310, None)),
           ("fqss_infer_ola_chunks", (None, q, p, 2, 1, 310, 100, 75, 100, 310, None)),
           ("fqss_infer_ola_chunks", (p, q, p, 2, 1, 310, 100, 75, 99, 310, None)),  # ld_chunk < seg
           ("fqss_infer_ola_chunks", (p, q, p, 2, 1, 310, 100, 75, 100, 309, None)),
           ("fqss_infer_ola_chunks", (p, q, p, 2, 1, 310, 100, 101, 100, 310, None))]
    for name, args in bad:
        with pytest.raises(_lib.FqssError, match=name):
            _lib.call(name, *args)
    assert bool((f == 0).all()) and bool((i == 0).all())
