"""The batched chunked-inference path on the GPU: `process.model_infer(chunk_batch=G)` and its four entry points (fqss_splitter2_rows,
fqss_chunk_gather, fqss_sisnr_chunks, fqss_infer_ola_chunks) against the chunk-by-chunk path they replace -- bit for bit where the
arithmetic is the same (splitter, overlap-add, re-ordering maps), within the bounds of tests/test_infer_batched_cpu.py against the
fp64 checkers of tests/helpers_infer_batched.py elsewhere."""
import numpy as np
import pytest
import torch

from tests import helpers_infer_batched as H
from tests.test_gpu_infer import T, _model

pytestmark = pytest.mark.gpu
SEG, OVERLAP = 1000, 0.25                 # on the 3100-sample mixture of tests/golden/infer.npz: 5 chunks, the last 100 samples long


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. splitter
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
def test_splitter2_rows_equals_stacked_splitter2(n):
    from fqss_amd import kernels as K
    x = torch.randn(5, n, generator=torch.Generator().manual_seed(n)) * 0.3
    x = (x * torch.tensor([1.0, 0.1, 1e-3, 7.0, 0.5])[:, None]).cuda()
    want = torch.cat([K.splitter2(x[b:b + 1]) for b in range(5)])
    out = torch.full((5, 2, n + 3), float("nan"), device="cuda")      # a NaN-guarded buffer: nothing is written past the rows
    ws = torch.zeros(5, device="cuda", dtype=torch.int32)
    from fqss_amd import _lib
    _lib.call("fqss_splitter2_rows", x.data_ptr(), out.data_ptr(), 5, n, ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    flat = out.reshape(-1)
    assert torch.equal(flat[:10 * n].view(5, 2, n), want) and bool(torch.isnan(flat[10 * n:]).all())
    assert torch.equal(ws.view(torch.float32), x.abs().amax(dim=1))
    assert torch.equal(K.splitter2_rows(x), want) and torch.equal(K.splitter2_rows(x.unsqueeze(1)), want)
    if n > 1:
        assert not torch.equal(K.splitter2(x), want)                  # rows at different levels: the global threshold differs


# ---- 2. overlap-add
@pytest.mark.parametrize("L,seg,overlap", H.GEOMETRIES + [(3100, 1000, 0.9)])
def test_infer_ola_chunks_equals_the_chunk_by_chunk_overlap_add(L, seg, overlap):
    from fqss_amd import kernels as K
    stride, N, ns = H.geometry(L, seg, overlap)
    for S, C in ((2, 1), (3, 2)):
        chunks, maps = H.ola_case(L, seg, overlap, S, C, seed=5, pad_chunks=1)
        cd, md = T(chunks).cuda(), T(maps).cuda()
        for mp in (md, None):
            out = torch.zeros(S, C, L, device="cuda")
            sw = torch.zeros(L, device="cuda")
            for k in range(N):
                K.infer_ola(cd[k, :, :, :ns[k]].contiguous(), None if mp is None else mp[k], out, sw, k * stride, ns[k], seg)
            K.infer_normalize(out, sw)
            got = K.infer_ola_chunks(cd, mp, L, stride)
            assert torch.equal(bits(got), bits(out)), (S, C, mp is not None, float((got - out).abs().max()))
            assert torch.equal(bits(K.infer_ola_chunks(cd, mp, L, stride)), bits(got))      # the same bits on a second run
            err = np.abs(got.cpu().numpy() - H.ola_ref(chunks, None if mp is None else maps, L, stride)).max()
            assert err <= 1e-6 * float(np.nanmax(np.abs(chunks))), err


# ---- 3. SI-SNR matrices and maps of a group in one launch
@pytest.mark.parametrize("S", [2, 3])
def test_sisnr_chunks_equals_per_chunk_sisnr_matrix(S):
    from fqss_amd import kernels as K
    L = 3100
    stride, N, ns = H.geometry(L, SEG, OVERLAP)
    ref, est = H.sisnr_case(L, SEG, OVERLAP, S, seed=6)
    db64, mp64, margin = H.sisnr_chunks_ref(est, ref, SEG, stride)
    assert margin >= H.MARGIN_DB, margin
    rd = torch.full((S, L + 5), float("nan"), device="cuda")
    rd[:, :L] = T(ref).cuda()
    rd = rd[:, :L]                                                    # pitched rows
    serial = [K.sisnr_matrix(T(est[k, :, :ns[k]]).cuda(), rd[:, k * stride:k * stride + ns[k]], want_map=True)[1] for k in range(N)]
    assert torch.equal(torch.stack(serial).cpu(), T(mp64))
    for G in (2, 5, 8):
        n_pad = -(-N // G) * G
        e = torch.full((n_pad, S, SEG), float("nan"), device="cuda")
        e[:N] = T(est).cuda()
        runs = []
        for _ in range(2):
            db = torch.full((n_pad, S, S), float("nan"), device="cuda")
            mp = torch.full((n_pad, S, 2), -7, device="cuda", dtype=torch.int32)
            for k0 in range(0, N, G):
                K.sisnr_chunks(e[k0:k0 + G], rd, stride, k0, db=db[k0:k0 + G], mp=mp[k0:k0 + G])
            runs.append((db, mp))
        (db, mp), (db2, mp2) = runs
        assert torch.equal(mp[:N], torch.stack(serial)), G
        np.testing.assert_allclose(db[:N].cpu().numpy(), db64, rtol=1e-5, atol=1e-4)
        assert torch.equal(bits(db[:N]), bits(db2[:N])) and torch.equal(mp, mp2)


def test_chunk_gather_on_the_gpu():
    from fqss_amd import kernels as K
    for L, seg, overlap in H.GEOMETRIES:
        stride, N, _ = H.geometry(L, seg, overlap)
        mix = np.random.RandomState(7).randn(1, L).astype(np.float32)
        for G, k0 in ((N + 3, 0), (2, N - 1)):                         # both run past the last chunk
            got = K.chunk_gather(T(mix).cuda(), seg, stride, k0, G)
            assert np.array_equal(got.cpu().numpy(), H.gather_ref(mix, seg, stride, k0, G)), (L, seg, overlap, G)


# ---- 4. model level
@pytest.fixture(scope="module")
def tiny(golden):
    """the tiny ConvTasNet of tests/golden/infer.npz, the fixture's mixture, a second mixture whose second half is 20 dB down (a
    global threshold would show), and for that one the chunk-by-chunk results and encoder inputs, computed once"""
    from fqss_amd.process import model_infer
    g = golden("infer")
    m = _model(g)
    mix, clean = T(g["mix"]).cuda(), T(g["clean"]).cuda()
    quiet = mix.clone()
    quiet[:, quiet.shape[-1] // 2:] *= 0.1
    seen = []
    hook = m.encoder.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().clone()))
    serial = dict(t=model_infer(m, quiet, n_srcs=2, segment=SEG, overlap=OVERLAP, target=clean).clone(),
                  nt=model_infer(m, quiet, n_srcs=2, segment=SEG, overlap=OVERLAP).clone())
    hook.remove()
    assert len(seen) == 10 and all(tuple(s.shape) == (1, 2, SEG) for s in seen)
    from fqss_amd.runtime import InferRunner
    return dict(g=g, m=m, run=InferRunner(m), mix=mix, clean=clean, quiet=quiet, serial=serial, enc_in=seen[:5])


def _callers(tiny):
    return (("module", tiny["m"]), ("runner", tiny["run"]))        # one runner for the module: one graph per chunk-batch shape


@pytest.mark.parametrize("G", [2, 5, 8])
def test_model_infer_chunk_batch_within_the_reference_bounds(tiny, G):
    """(a) against the reference's own chunked results, the three bounds of test_model_infer_matches_the_reference"""
    from fqss_amd.process import model_infer
    for name, model in _callers(tiny):
        for key, tgt in (("chunked", tiny["clean"]), ("chunked_nt", None)):
            got = model_infer(model, tiny["mix"], n_srcs=2, segment=SEG, overlap=OVERLAP, target=tgt, chunk_batch=G)
            want = tiny["g"][key]
            assert tuple(got.shape) == want.shape
            err = np.abs(got.cpu().numpy() - want)
            scale = np.abs(want).max()
            stats = (name, key, float(err.max() / scale), float(np.sqrt(np.mean(err ** 2)) / scale), float(np.mean(err > 1e-3 * scale)))
            print(stats)
            assert stats[2] <= 0.08 and stats[3] <= 5e-3 and stats[4] <= 0.05, stats


@pytest.mark.parametrize("G", [2, 5, 8])
def test_every_chunk_meets_the_encoder_as_on_the_chunk_by_chunk_path(tiny, G):
    """(b) the encoder's input -- the splitter's output -- of every chunk, bit for bit: a threshold taken over the whole batch shows
    here whatever else differs"""
    from fqss_amd.process import model_infer
    seen = []
    hook = tiny["m"].encoder.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().clone()))
    try:
        model_infer(tiny["m"], tiny["quiet"], n_srcs=2, segment=SEG, overlap=OVERLAP, chunk_batch=G)
    finally:
        hook.remove()
    assert [tuple(s.shape) for s in seen] == [(G, 2, SEG)] * -(-5 // G)
    rows = torch.cat(seen)
    for k in range(5):
        assert torch.equal(bits(rows[k]), bits(tiny["enc_in"][k][0])), k
    for k in range(5, rows.shape[0]):                                  # the padding rows repeat the last chunk
        assert torch.equal(bits(rows[k]), bits(tiny["enc_in"][4][0]))


def test_eval_forward_is_batch_invariant(tiny):
    """what (c) below rests on: an item's output does not depend on what else is in the batch (both rows share a maximum, so the
    global splitter agrees)"""
    m = tiny["m"]
    x = tiny["quiet"][:, :SEG].reshape(1, 1, SEG).contiguous()
    with torch.no_grad():
        one = m(x).clone()
        for B in (2, 5, 8):
            many = m(x.repeat(B, 1, 1))
            for b in range(B):
                assert torch.equal(bits(many[b]), bits(one[0])), (B, b)


@pytest.mark.parametrize("G", [2, 5, 8])
def test_model_infer_chunk_batch_equals_the_chunk_by_chunk_path(tiny, G):
    """(c) the same bits as chunk_batch=None, as a plain module and through InferRunner's graphs, with and without a target"""
    from fqss_amd.process import model_infer
    for name, model in _callers(tiny):
        for key, tgt in (("t", tiny["clean"]), ("nt", None)):
            got = model_infer(model, tiny["quiet"], n_srcs=2, segment=SEG, overlap=OVERLAP, target=tgt, chunk_batch=G)
            want = tiny["serial"][key]
            assert got.shape == want.shape
            assert torch.equal(bits(got), bits(want)), (name, key, float((got - want).abs().max()))


def test_infer_runner_keeps_per_item_and_global_graphs_apart(tiny):
    """(d) one shape served both ways alternately: two graphs, each returning its own eager result"""
    from fqss_amd import ops
    from fqss_amd.runtime import InferRunner
    m = tiny["m"]
    run = InferRunner(m)
    x = torch.stack([tiny["quiet"][:, :SEG], tiny["quiet"][:, 2000:2000 + SEG]]).contiguous()      # a loud and a quiet row
    with torch.no_grad():
        want_global = m(x).clone()
        with ops.split_per_item(True):
            want_rows = m(x).clone()
    assert not torch.equal(want_global, want_rows)
    for _ in range(2):
        assert torch.equal(run(x), want_global)
        with ops.split_per_item(True):
            assert torch.equal(run(x), want_rows)
    assert len(run._graphs) == 2


# ---- 5. refusals
def test_refusals_on_the_gpu(tiny):
    from fqss_amd import _lib, ops, process
    m = tiny["m"]
    for G in (0, -1):
        with pytest.raises(ValueError, match="chunk_batch"):
            process.model_infer(m, tiny["mix"], n_srcs=2, segment=SEG, chunk_batch=G)
    with pytest.raises(NotImplementedError, match="one-channel"):
        process.model_infer(m, tiny["mix"].repeat(2, 1), n_srcs=2, segment=SEG, chunk_batch=2)
    spec = torch.randn(2, 2, 8, 50, device="cuda")                     # HTDemucs-style inputs: a spectrogram and a stereo waveform
    with ops.split_per_item(True):
        for x, kw in ((spec, dict()), (spec[:, :, 0], dict(normalize=False))):
            with pytest.raises(NotImplementedError, match="split_per_item"):
                process.preprocess(x, n_splitter=2, **kw)
    assert process.preprocess(spec, n_splitter=2).shape == (2, 4, 8, 50)      # outside the block: as before
    f = torch.zeros(4096, device="cuda")
    i = torch.zeros(64, device="cuda", dtype=torch.int32)
    p, q, st = f.data_ptr(), i.data_ptr(), torch.cuda.current_stream().cuda_stream
    bad = [("fqss_chunk_gather", (None, p, 3100, 1000, 750, 0, 2, st)),
           ("fqss_chunk_gather", (p, p, 3100, 1000, 750, 5, 2, st)),
           ("fqss_chunk_gather", (p, p, 3100, 1000, 1001, 0, 2, st)),
           ("fqss_chunk_gather", (p, p, 3100, 1000, 750, 0, 0, st)),
           ("fqss_splitter2_rows", (p, p, 2, 100, None, st)),
           ("fqss_splitter2_rows", (p, p, 2, 0, q, st)),
           ("fqss_sisnr_chunks", (p, None, p, q, 2, 2, 100, 75, 0, 310, 310, st)),
           ("fqss_sisnr_chunks", (p, p, p, q, 2, 17, 100, 75, 0, 310, 310, st)),
           ("fqss_sisnr_chunks", (p, p, p, q, 2, 2, 100, 75, 0, 310, 309, st)),
           ("fqss_sisnr_chunks", (p, p, p, q, 0, 2, 100, 75, 0, 310, 310, st)),
           ("fqss_infer_ola_chunks", (p, q, None, 2, 1, 310, 100, 75, 100, 310, st)),
           ("fqss_infer_ola_chunks", (p, q, p, 2, 1, 310, 100, 75, 99, 310, st)),
           ("fqss_infer_ola_chunks", (p, q, p, 2, 1, 310, 100, 0, 100, 310, st)),
           ("fqss_infer_ola_chunks", (p, q, p, 2, 1, 310, 100, 101, 100, 310, st))]
    for name, args in bad:
        with pytest.raises(_lib.FqssError, match=name):
            _lib.call(name, *args)
    torch.cuda.synchronize()
    assert bool((f == 0).all()) and bool((i == 0).all())
