"""`kernels.hd_augment_mix` (fqss_hd_augment_mix, csrc/data_ops.hip) against its statement in include/fqss.h, written here with torch
CPU fp32 ops, one operation per line, the mixture summed explicitly from left to right.  Every operation is one correctly rounded
fp32 operation on both sides, so the gate is torch.equal: there is no tolerance."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def statement(pcm, T_out, src_b, off, flip, gain, mean=None, std=None):
    """pcm int16 [B, S, T_in, C] (CPU) -> (mix [B, C, T_out], sources [B, S, C, T_out])"""
    B, S, T_in, C = pcm.shape
    sources = torch.empty(B, S, C, T_out, dtype=torch.float32)
    for b in range(B):
        for s in range(S):
            bs, o = int(src_b[b, s]), int(off[b, s])
            for c in range(C):
                cs = 1 - c if (C == 2 and int(flip[b, s])) else c
                v = pcm[bs, s, o:o + T_out, cs].to(torch.float32)
                v = v * torch.tensor(2.0 ** -15, dtype=torch.float32)
                if mean is not None:
                    v = v - mean[bs]
                    v = v / std[bs]
                v = v * gain[b, s]
                sources[b, s, c] = v
    mix = sources[:, 0].clone()
    for s in range(1, S):
        mix = mix + sources[:, s]
    return mix, sources


def random_pcm(B, S, T_in, C, seed):
    g = torch.Generator().manual_seed(seed)
    pcm = torch.randint(-32768, 32768, (B, S, T_in, C), generator=g, dtype=torch.int32).to(torch.int16)
    pcm.view(-1)[:4] = torch.tensor([-32768, 32767, 0, -1], dtype=torch.int16)
    pcm.view(-1)[-2:] = torch.tensor([32767, -32768], dtype=torch.int16)
    return pcm


def random_table(B, S, T_in, T_out, seed, C=2):
    g = torch.Generator().manual_seed(seed)
    src_b = torch.stack([torch.randperm(B, generator=g) for _ in range(S)], dim=1)
    off = torch.randint(0, T_in - T_out + 1, (B, S), generator=g)
    flip = torch.randint(0, 2, (B, S), generator=g) if C == 2 else torch.zeros(B, S, dtype=torch.int64)
    gain = (0.25 + torch.rand(B, S, generator=g)) * (2 * torch.randint(0, 2, (B, S), generator=g) - 1)
    mean = (torch.rand(B, generator=g) - 0.5) * 0.02
    std = 0.05 + torch.rand(B, generator=g) * 0.3
    return src_b, off, flip, gain.float(), mean.float(), std.float()


def run(pcm, T_out, src_b, off, flip, gain, mean=None, std=None, **kw):
    from fqss_amd import kernels as K
    mix, sources = K.hd_augment_mix(pcm.cuda(), T_out, src_b, off, flip, gain, mean, std, **kw)
    torch.cuda.synchronize()
    return mix.cpu(), sources.cpu()


def check(pcm, T_out, *table):
    want_mix, want_src = statement(pcm, T_out, *table)
    mix, src = run(pcm, T_out, *table)
    assert mix.shape == want_mix.shape and src.shape == want_src.shape
    assert torch.isfinite(src).all() and torch.equal(src, want_src)
    assert torch.equal(mix, want_mix)


def test_main_case():
    """(a) B 4, S 3, stereo, 1064 -> 1003 samples (no multiple of a vector width): offsets 0, 61 and odd ones, both kinds of flip,
    gains with a negative one, 1.0 and 0.25, a remix table that is not the identity, PCM over the whole int16 range"""
    B, S, T_in, T_out = 4, 3, 1064, 1003
    pcm = random_pcm(B, S, T_in, 2, seed=1)
    src_b = torch.tensor([[1, 0, 3], [0, 2, 2], [3, 1, 0], [2, 3, 1]])
    off = torch.tensor([[0, 61, 17], [33, 0, 61], [1, 60, 5], [61, 7, 0]])
    flip = torch.tensor([[0, 1, 1], [1, 0, 0], [0, 0, 1], [1, 1, 0]])
    gain = torch.tensor([[-0.7, 1.0, 0.25], [1.25, -1.0, 0.3], [0.9, 1.0, -0.25], [1.0, 0.61, -1.1]], dtype=torch.float32)
    mean = torch.tensor([0.003, -0.011, 0.0, 0.02], dtype=torch.float32)
    std = torch.tensor([0.11, 0.31, 1.0, 0.07], dtype=torch.float32)
    check(pcm, T_out, src_b, off, flip, gain, mean, std)
    check(pcm, T_out, src_b, off, flip, gain)                     # the same table with normalise off


def test_smallest_case():
    """(b) one mono sample"""
    pcm = torch.tensor([-12345], dtype=torch.int16).reshape(1, 1, 1, 1)
    one = torch.zeros(1, 1, dtype=torch.int64)
    check(pcm, 1, one, one, one, torch.tensor([[-0.5]]), torch.tensor([0.01]), torch.tensor([0.2]))


def test_eight_sources_several_blocks():
    """(c) B 2, S 8, 4097 samples: the longest sum, more than one block per item"""
    B, S, T_in, T_out = 2, 8, 4200, 4097
    pcm = random_pcm(B, S, T_in, 2, seed=2)
    check(pcm, T_out, *random_table(B, S, T_in, T_out, seed=3))


@pytest.mark.parametrize("C,S,T_in,T_out", [(2, 4, 4399, 4096), (2, 3, 1100, 1004), (1, 2, 1061, 1000), (1, 3, 1064, 1003)])
def test_wide_store_path_and_mono(C, S, T_in, T_out):
    """T_out a multiple of 4 takes the 16-byte-store kernels (stereo and mono), with offsets that leave the input at every alignment
    a frame allows; mono also on the one-sample-per-lane path"""
    B = 3
    pcm = random_pcm(B, S, T_in, C, seed=4)
    src_b, off, flip, gain, mean, std = random_table(B, S, T_in, T_out, seed=5, C=C)
    off[0, :min(S, 4)] = torch.tensor([0, 1, 2, 3])[:min(S, 4)]
    off[1, 0] = T_in - T_out
    check(pcm, T_out, src_b, off, flip, gain, mean, std)


def test_identity_table_is_the_decoded_file():
    """(d) identity table, normalise off: pcm / 32768 transposed to planar, and its sum"""
    from fqss_amd.train_env.htdemucs_musdbhq.wav_dataset import identity_table
    B, S, T = 2, 4, 777
    pcm = random_pcm(B, S, T, 2, seed=6)
    mix, src = run(pcm, T, *identity_table(B, S))
    want = (pcm.to(torch.float32) / 32768.0).permute(0, 1, 3, 2).contiguous()
    assert torch.equal(src, want)
    assert torch.equal(mix, ((want[:, 0] + want[:, 1]) + want[:, 2]) + want[:, 3])


def test_every_output_is_written_and_the_call_repeats_bit_for_bit():
    """(e) the same call twice into NaN-filled outputs: identical bits, no NaN left"""
    B, S, T_in, T_out = 4, 3, 1064, 1003
    pcm = random_pcm(B, S, T_in, 2, seed=7)
    table = random_table(B, S, T_in, T_out, seed=8)
    outs = []
    for _ in range(2):
        src = torch.full((B, S, 2, T_out), float("nan"), device="cuda")
        mix = torch.full((B, 2, T_out), float("nan"), device="cuda")
        got = run(pcm, T_out, *table, sources=src, mix=mix)
        assert got[0].data_ptr() != 0 and not torch.isnan(got[0]).any() and not torch.isnan(got[1]).any()
        outs.append(got)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    want_mix, want_src = statement(pcm, T_out, *table)
    assert torch.equal(outs[0][0], want_mix) and torch.equal(outs[0][1], want_src)


def test_bad_table_launches_nothing_on_the_device():
    """with the device present too: a row out of range is a ValueError and the poisoned outputs stay untouched"""
    from fqss_amd import kernels as K
    pcm = random_pcm(2, 2, 64, 2, seed=9).cuda()
    src = torch.full((2, 2, 2, 60), float("nan"), device="cuda")
    mix = torch.full((2, 2, 60), float("nan"), device="cuda")
    z = torch.zeros(2, 2, dtype=torch.int64)
    with pytest.raises(ValueError, match="off"):
        K.hd_augment_mix(pcm, 60, z, z + 5, z, torch.ones(2, 2), sources=src, mix=mix)
    with pytest.raises(ValueError, match="src_b"):
        K.hd_augment_mix(pcm, 60, z + 2, z, z, torch.ones(2, 2), sources=src, mix=mix)
    torch.cuda.synchronize()
    assert torch.isnan(src).all() and torch.isnan(mix).all()
