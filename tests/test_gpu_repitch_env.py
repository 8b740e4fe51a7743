"""The WAV dataset of the htdemucs env with `augment.repitch` on (wav_dataset.WavStems.batch: upload, kernels.hd_repitch,
kernels.hd_augment_mix) on a generated two-track tree of 16-bit stereo stems."""
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SR, SRC = 44100, ["a", "b", "c"]
AUG = {"shift_same": False, "flip": True, "remix": {"proba": 1, "group_size": 2}, "scale": {"proba": 1, "min": 0.25, "max": 1.25}}


def test_batches_with_repitch(tmp_path):
    from fqss_amd import kernels as K
    from fqss_amd.train_env.htdemucs_musdbhq import wav_dataset as W
    rng = np.random.default_rng(1)
    for i in range(2):
        for s in SRC:
            x = np.cumsum(rng.standard_normal((int((2 + i) * SR), 2)) * 300, axis=0).clip(-30000, 30000).astype("<i2")
            path = tmp_path / f"track{i}" / (s + ".wav")
            path.parent.mkdir(exist_ok=True)
            with wave.open(str(path), "wb") as w:
                w.setnchannels(2), w.setsampwidth(2), w.setframerate(SR)
                w.writeframes(x.tobytes())
    tracks = [str(tmp_path / f"track{i}") for i in range(2)]
    make = lambda proba: W.WavStems(tracks, SRC, SR, 2, segment=0.4, shift=0.05, normalize=True, train=True,
                                    augment=dict(AUG, repitch={"engine": "wsola", "proba": proba, "max_tempo": 12, "same": False}))
    ds, idx = make(1), W.SeededBatch([3, 40, 11, 60], 77)
    seg, stride = int(SR * 0.4), int(SR * 0.05)
    assert (ds.T_in, ds.T_rp, ds.T_out) == (seg, int(0.88 * seg), int(0.88 * seg) - stride)
    mix, src = ds.batch(idx)
    assert mix.shape == (4, 2, ds.T_out) and src.shape == (4, 3, 2, ds.T_out)
    again = ds.batch(idx)
    assert torch.equal(mix, again[0]) and torch.equal(src, again[1])                     # a function of the seed
    assert torch.equal(mix, (src[:, 0] + src[:, 1]) + src[:, 2])                         # the left-to-right sum, as without repitch
    pcm, table, mean, std, rp = ds.host_batch_repitch(idx)
    off_ds = make(0)
    pcm0, table0, _, _ = off_ds.host_batch(idx)
    assert torch.equal(pcm, pcm0) and all(torch.equal(a, b) for a, b in zip(table, table0))
    assert bool(rp.on.all()) and len(rp.pitch.unique()) > 1 and not torch.equal(rp.A, rp.A[:, :1].expand(4, 3))
    by_hand = K.hd_augment_mix(K.hd_repitch(pcm.cuda(), ds.T_rp, rp.on, rp.pitch, rp.A), ds.T_out, *table, mean, std)
    assert torch.equal(mix, by_hand[0]) and torch.equal(src, by_hand[1])                # the same launches by hand
    assert (off_ds.T_rp, off_ds.T_out) == (seg, seg - stride) and off_ds.host_batch_repitch(idx)[4] is None
    mix0, src0 = off_ds.batch(idx)
    want = K.hd_augment_mix(pcm0.cuda(), seg - stride, *table0, mean, std)
    assert torch.equal(mix0, want[0]) and torch.equal(src0, want[1])                    # proba 0: the path without repitch, bit for bit
