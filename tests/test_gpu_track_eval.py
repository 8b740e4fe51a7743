"""GPU: track evaluation of the HTDemucs recipe (csrc/track_eval.hip -> kernels -> process.preprocess / model_infer / calc_nsdr -> val.py)
against the statements of include/fqss.h written in NumPy: fp64 for the sums, float32 arithmetic where a statement is an exact IEEE
operation (then bit for bit), the chunk-by-chunk path where the batched one must reproduce it."""
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def within_one_ulp(got, want):
    """|got - fp32(want)| <= one fp32 ulp at want: both sides round an fp64 value once, the fp64 values differ by ~1e-16 relative"""
    return abs(float(got) - float(np.float32(want))) <= float(np.spacing(np.abs(np.float32(want))))


def nsdr_np(ref, est):
    """calc_nsdr of the reference over the last two dimensions, fp64"""
    r, e = ref.astype(np.float64), est.astype(np.float64)
    return 10.0 * np.log10(((r * r).sum((-2, -1)) + 1e-7) / (((r - e) ** 2).sum((-2, -1)) + 1e-7))


class Stub(torch.nn.Module):
    """[B, C, T] -> [B, 3, C, T]: per-source scaled and shifted copies, element by element (the batch size cannot change a bit)"""
    n_srcs, n_splitter, audio_channels, sources = 3, 1, 2, ["drums", "bass", "vocals"]

    def forward(self, x):
        return torch.stack([x * 0.5 + 0.25, x * -1.5, x + 1.0], dim=1)


# ---- 1. fqss_track_stats
@pytest.mark.parametrize("C,L,offset", [(C, L, 0.0) for C in (1, 2) for L in (2, 4095, 3 * 4096 + 1)] + [(2, 3 * 4096 + 1, 1000.0)])
def test_track_stats_against_fp64(C, L, offset):
    from fqss_amd import kernels as K
    assert K.TRACK_TILE == 4096
    x = (np.random.default_rng(L + C).standard_normal((C, L)) + offset).astype(np.float32)
    m = (x.sum(0, dtype=np.float32) / np.float32(C)).astype(np.float64)        # C <= 2: one fp32 addition, channel order
    want = (m.mean(), m.std(ddof=1))
    dense = torch.from_numpy(x).cuda()
    padded = K.empty_act((C, L), "cuda")                                       # 16-byte rows: the 16-byte load form
    padded.copy_(dense)
    got = K.track_stats(dense).cpu()
    print(f"C {C} L {L}: mean {got[0]:.9g} (fp64 {want[0]:.17g}), std {got[1]:.9g} (fp64 {want[1]:.17g})")
    assert torch.equal(K.track_stats(padded).cpu(), got), "the two load forms add in one order"
    assert within_one_ulp(got[0], want[0]) and within_one_ulp(got[1], want[1])
    assert torch.isnan(K.track_stats(dense[:, :1])[1])                         # L = 1: std NaN, as torch


# ---- 2. fqss_chunk_gather_mc
def gather_np(x, seg, stride, k0, G, stats):
    C, L = x.shape
    N, out = -(-L // stride), np.zeros((G, C, seg), np.float32)
    for g in range(G):
        k = min(k0 + g, N - 1)
        v = x[:, k * stride:k * stride + seg]
        out[g, :, :v.shape[1]] = v if stats is None else (v - stats[0]) / stats[1]      # float32 arithmetic
    return out


@pytest.mark.parametrize("k0", [0, 3])
@pytest.mark.parametrize("stride,ld", [(6, 20), (6, 23), (4, 32)])            # dense, an unaligned row stride, the 16-byte form
def test_chunk_gather_mc_bit_for_bit(stride, ld, k0):
    from fqss_amd import kernels as K
    x = np.random.default_rng(ld).standard_normal((2, 20)).astype(np.float32)
    stats = np.array([0.3, 1.7], np.float32)
    mix = torch.zeros(2, ld, device="cuda")[:, :20]
    mix.copy_(torch.from_numpy(x))
    for st in (None, stats):
        got = K.chunk_gather_mc(mix, 8, stride, k0, 3, stats=None if st is None else torch.from_numpy(st).cuda())
        assert np.array_equal(got.cpu().numpy(), gather_np(x, 8, stride, k0, 3, st)), (stride, ld, k0, st is None)
    assert np.array_equal(K.chunk_gather_mc(mix[:1], 8, stride, k0, 3).cpu().numpy(), gather_np(x[:1], 8, stride, k0, 3, None))      # C = 1


# ---- 3. the per-item splitter
def same(a, b):
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def test_splitter2_raw_rows_is_the_global_splitter_per_item():
    from fqss_amd import kernels as K
    x = torch.randn(3, 1023, device="cuda") * torch.tensor([1.0, 0.0, 30.0], device="cuda")[:, None]
    got = K.splitter2_raw_rows(x)
    for b in range(3):
        assert same(got[b:b + 1], K.splitter2(x[b:b + 1], normalize=False)), b
    assert bool(got[1].isnan().all()) and not bool(got[0].isnan().any()) and not bool(got[2].isnan().any())


@pytest.mark.parametrize("normalize", [True, False])
def test_preprocess_per_item_on_multi_dimensional_inputs(normalize):
    from fqss_amd import ops, process
    x = torch.randn(2, 2, 8, 50, device="cuda") * torch.tensor([1.0, 0.05], device="cuda")[:, None, None, None]
    with ops.split_per_item("items"):
        got = process.preprocess(x, n_splitter=2, normalize=normalize)
    want = torch.cat([process.preprocess(x[b:b + 1], n_splitter=2, normalize=normalize) for b in range(2)])
    assert got.shape == (2, 4, 8, 50) and torch.equal(got, want)
    assert not torch.equal(got, process.preprocess(x, n_splitter=2, normalize=normalize))      # the global threshold is another result


def test_htdemucs_pre_process_per_item():
    from fqss_amd import ops
    from fqss_amd.quantization.qat.models.htdemucsq import HTDemucsQ
    torch.manual_seed(0)
    m = HTDemucsQ(sources=["a", "b"], audio_channels=2, channels=8, nfft=2048, depth=4, bottom_channels=16, t_layers=3, t_heads=2).cuda().train()
    m.set_splitter_combiner(2, 2)
    mix = torch.randn(2, 2, 8192, device="cuda") * torch.tensor([1.0, 0.1], device="cuda")[:, None, None]
    with ops.split_per_item("items"):
        both = m.pre_process(mix)
        for b in range(2):
            for got, want in zip(both, m.pre_process(mix[b:b + 1])):
                assert torch.equal(got[b:b + 1], want), b


# ---- 4. stereo chunk batches
@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("overlap", [0.25, 0.0])          # hops of 75 (14 chunks) and of seg = 100 (11 chunks) over 1030 samples
def test_stereo_chunk_batches_equal_the_chunk_by_chunk_path(overlap, G):
    from fqss_amd import kernels as K
    from fqss_amd.process import model_infer
    torch.manual_seed(1)
    stub, mix = Stub(), torch.randn(2, 1030, device="cuda") * 0.3 + 0.1
    want = model_infer(stub, mix, segment=100, overlap=overlap)
    got = model_infer(stub, mix, segment=100, overlap=overlap, chunk_batch=G)
    assert got.shape == (3, 2, 1030) and torch.equal(got, want)
    stats = K.track_stats(mix)
    norm = ((mix.cpu() - stats.cpu()[0]) / stats.cpu()[1]).cuda()             # IEEE fp32 subtraction and division, on the host
    want = model_infer(stub, norm, segment=100, overlap=overlap) * stats[1] + stats[0]
    assert torch.equal(model_infer(stub, mix, segment=100, overlap=overlap, chunk_batch=G, stats=stats), want)
    with pytest.raises(ValueError, match="stats"):                             # stats belongs to the batched path
        model_infer(stub, mix, segment=100, overlap=overlap, stats=stats)


# ---- 5. fqss_nsdr
@pytest.mark.parametrize("N", [1, 4097, 2 * 4096 + 5])
def test_nsdr_against_fp64(N):
    from fqss_amd import kernels as K
    from fqss_amd.process import calc_nsdr
    rng = np.random.default_rng(N)
    ref = rng.standard_normal((3, N)).astype(np.float32)
    est = (ref + 0.1 * rng.standard_normal((3, N))).astype(np.float32)
    est[1] = ref[1]                                                            # den = 0
    ref[2] = 0.0                                                               # a silent reference
    want = nsdr_np(ref[:, None], est[:, None])
    got = K.nsdr(torch.from_numpy(est).cuda(), torch.from_numpy(ref).cuda()).cpu().numpy()
    print(f"N {N}: {got} (fp64 {want}), max |diff| {np.abs(got - want).max():.3g} dB")
    assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-9
    if N == 1:
        return
    r4, e4 = torch.from_numpy(ref[:, :N - 1]).cuda().view(3, 1, 2, -1), torch.from_numpy(est[:, :N - 1]).cuda().view(3, 1, 2, -1)
    got = calc_nsdr(r4, e4)                                                     # [..., C, L]: the leading dimensions are the rows
    assert got.shape == (3, 1) and np.abs(got.cpu().numpy() - nsdr_np(r4.cpu().numpy(), e4.cpu().numpy())).max() <= 1e-9


# ---- 6. val.py
@pytest.mark.parametrize("sub,G", [("", None), ("test", 2)])
def test_val_musdbhq_nsdr(tmp_path, monkeypatch, capsys, sub, G):
    import yaml
    from fqss_amd import kernels as K
    from fqss_amd import val
    from fqss_amd.process import model_infer
    rng, stub, want = np.random.default_rng(7), Stub().cuda(), []
    for name in ("t0", "t1"):
        folder = tmp_path / "db" / sub / name
        folder.mkdir(parents=True)
        pcm = {s: rng.integers(-9000, 9000, (8820, 2)).astype("<i2") for s in ["mixture"] + Stub.sources}      # 0.2 s
        for s, a in pcm.items():
            with wave.open(str(folder / (s + ".wav")), "wb") as w:
                w.setnchannels(2), w.setsampwidth(2), w.setframerate(44100), w.writeframes(a.tobytes())
        mix = torch.from_numpy(pcm["mixture"].T.astype(np.float32) / 32768.0).cuda()
        st = K.track_stats(mix)
        sep = model_infer(stub, mix, segment=4000, chunk_batch=G, stats=st) if G else \
            model_infer(stub, (mix - st[0]) / st[1], segment=4000) * st[1] + st[0]
        refs = np.stack([pcm[s].T.astype(np.float32) / 32768.0 for s in Stub.sources])
        want.append(nsdr_np(refs, sep.cpu().numpy()))
    want = np.mean(want, axis=0)
    cfg = dict(model_cfg=dict(name="stub", quantization=dict(qat=True)), dataset_cfg=dict(name="musdbhq"),
               testing_cfg=dict(test_dir=str(tmp_path / "db"), NSDR=True, segment_samples=4000, overlap=0.25, chunk_batch=G))
    monkeypatch.setattr(val, "create_pretrained_model", lambda model_cfg: Stub())
    monkeypatch.setattr(sys, "argv", ["val"])
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    got = val.val(["-y", str(tmp_path / "cfg.yaml")])
    print(got, want)
    assert len(got) == 4 and np.abs(np.array(got[1:]) - want).max() <= 1e-9 and abs(got[0] - want.mean()) <= 1e-9
    assert "NSDR={:0.2f},NSDR_DRUMS={:0.2f},NSDR_BASS={:0.2f},SNDR_VOCALS={:0.2f}".format(*got) in capsys.readouterr().out
    cfg["testing_cfg"]["NSDR"] = False
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    with pytest.raises(NotImplementedError, match="museval"):
        val.val(["-y", str(tmp_path / "cfg.yaml")])
