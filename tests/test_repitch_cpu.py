"""Host side of the repitch augmentation of the htdemucs env (wav_dataset.draw_repitch / check_augment_cfg / the lengths,
kernels.repitch_taps) and the sanity of the NumPy checker the GPU test compares against (tests/helpers_repitch.py).  No device."""
import wave

import numpy as np
import pytest
import torch

from tests.helpers_repitch import repitch_stream

CFG = {"shift_same": False, "flip": True, "remix": {"proba": 1, "group_size": 4}, "scale": {"proba": 1, "min": 0.25, "max": 1.25}}
RP = {"engine": "wsola", "proba": 1, "max_pitch": 2, "max_tempo": 12, "tempo_std": 5, "same": True}


def test_the_chain_table_does_not_depend_on_the_repitch_switch():
    from fqss_amd.train_env.htdemucs_musdbhq.wav_dataset import draw_augment
    for seed in range(5):
        a, b = (draw_augment(8, 4, 2, 441, dict(CFG, repitch=dict(RP, proba=p)), torch.Generator().manual_seed(seed)) for p in (0, 1))
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_draw_repitch_ranges_same_and_proba():
    from fqss_amd import kernels as K
    from fqss_amd.train_env.htdemucs_musdbhq.wav_dataset import draw_repitch
    draw = lambda seed, **over: draw_repitch(64, 4, {"repitch": dict(RP, **over)}, torch.Generator().manual_seed(seed))
    t = draw(0)
    assert all(torch.equal(x, x[:, :1].expand(64, 4)) for x in t)                          # same: one draw per item
    assert bool(t.on.all()) and set(t.pitch.unique().tolist()) == {-2, -1, 0, 1, 2}
    assert float(t.tempo.abs().max()) <= 12 and float(t.tempo.std()) > 3
    assert t.A.tolist() == [[K.repitch_A(p, v) for p, v in zip(ps, vs)] for ps, vs in zip(t.pitch.tolist(), t.tempo.tolist())]
    wide = draw(0, tempo_std=50)
    assert float(wide.tempo.abs().max()) == 12 and int((wide.tempo.abs() == 12).sum()) > 64      # the clamp
    per = draw(0, same=False).pitch
    assert not torch.equal(per, per[:, :1].expand(64, 4))                                  # per stem
    some = draw(1, proba=0.2, same=False)
    assert 20 < int(some.on.sum()) < 90
    off = some.on == 0
    assert not some.pitch[off].any() and not some.tempo[off].any() and bool((some.A[off] == 65536).all())
    with pytest.raises(ValueError, match="proba"):
        draw(0, proba=0)


def test_lengths_and_refusals(tmp_path):
    from fqss_amd.train_env.htdemucs_musdbhq import wav_dataset as W
    assert W.repitch_length(441000, {"repitch": RP}) == 388080 and W.repitch_length(441000, {"repitch": dict(RP, proba=0)}) == 441000
    for s in ("a", "b"):
        path = tmp_path / "t0" / (s + ".wav")
        path.parent.mkdir(exist_ok=True)
        with wave.open(str(path), "wb") as w:
            w.setnchannels(2), w.setsampwidth(2), w.setframerate(44100)
            w.writeframes(np.zeros((1000, 2), "<i2").tobytes())
    kw = dict(sources=["a", "b"], samplerate=44100, channels=2, segment=10, shift=1)
    for train in (True, False):
        ds = W.WavStems([str(tmp_path / "t0")], train=train, augment={"repitch": RP}, **kw)
        assert (ds.T_rp, ds.T_out, ds.T_in) == (388080, 343980, 441000 if train else 343980)
    for bad in (dict(max_pitch=3), dict(max_tempo=25), dict(max_tempo=24)):               # 24 with two semitones: a stretch below 0.70
        with pytest.raises(ValueError, match=r"augment\.repitch"):
            W.check_augment_cfg({"repitch": dict(RP, **bad)})
    W.check_augment_cfg({"repitch": dict(RP, max_tempo=24, max_pitch=0)})
    with pytest.raises(ValueError, match="engine"):
        W.check_augment_cfg({"repitch": dict(RP, engine="rubberband")})


def test_every_phase_sums_to_exactly_two_to_the_fifteen():
    from fqss_amd import kernels as K
    assert sorted(K.REPITCH_RATIOS) == [-2, -1, 0, 1, 2]
    for P, Q in K.REPITCH_RATIOS.values():
        hq = K.repitch_taps(P, Q)
        assert hq.shape == (Q, K.RP_J) and (hq.sum(axis=1) == 1 << 15).all() and int(np.abs(hq).sum(axis=1).max()) < 1 << 17
    assert K.repitch_table().shape == (K.RP_HQ_ROWS, K.RP_J) and K.repitch_taps(1, 1)[0, K.RP_J // 2 - 1] == 1 << 15


def test_checker_identity_and_spectral_peaks():
    """pitch 0 / tempo 0 is a crop; pitch +2 moves a 1 kHz tone to 1000 * 55 / 49 Hz; tempo +12 leaves it at 1000 Hz (one FFT bin)"""
    from fqss_amd import kernels as K
    x = np.random.default_rng(0).integers(-20000, 20000, (20000, 2)).astype(np.int16)
    y, p = repitch_stream(x, 17600, 1, 1, K.repitch_A(0, 0), K.repitch_taps(1, 1))
    assert np.array_equal(y, x[:17600]) and p == [1536 * m for m in range(len(p))]
    tone = np.rint(8000 * np.sin(2 * np.pi * 1000.0 * np.arange(20000) / 44100))[:, None].astype(np.int16)
    for pitch, tempo, want in ((2, 0.0, 1000 * 55 / 49), (0, 12.0, 1000.0)):
        P, Q = K.REPITCH_RATIOS[pitch]
        y, _ = repitch_stream(tone, 17600, P, Q, K.repitch_A(pitch, tempo), K.repitch_taps(P, Q))
        y = y[2000:16000, 0].astype(np.float64)                                            # clear of the edges and of the track's end
        peak = np.argmax(np.abs(np.fft.rfft(y * np.hanning(len(y))))) * 44100 / len(y)
        assert abs(peak - want) <= 44100 / len(y), (pitch, tempo, peak)
