"""GPU: frame-wise SDR (fqss_frame_sdr in include/fqss.h: csrc/track_eval.hip -> kernels.frame_sdr -> process.calc_frame_sdr -> val.py)
against its statement in fp64 NumPy.  Both sides add fp64 squares of the same fp32 samples (at most 2 x 1024 per window here: their
orders differ by ~1e-14 relative, 1e-13 dB), so the 1e-9 dB gate of fqss_nsdr's test holds the kernel to its statement."""
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def frame_sdr_np(ref, est, win, hop):
    """the statement: (med [S], frames [S, W]) of ref, est [S, C, L]"""
    S, C, L = ref.shape
    W = (L - win) // hop + 1 if L >= win else 0
    r, e, frames = ref.astype(np.float64), est.astype(np.float64), np.full((S, W), np.nan)
    for w in range(W):
        rw, ew = r[:, :, w * hop:w * hop + win], e[:, :, w * hop:w * hop + win]
        if (rw != 0).any((1, 2)).all() and (ew != 0).any((1, 2)).all():
            num, den = (rw * rw).sum((1, 2)), ((rw - ew) ** 2).sum((1, 2))
            frames[:, w] = np.where(den == 0, np.inf, 10.0 * np.log10(num / np.where(den == 0, 1.0, den)))
    return np.array([np.nanmedian(row) if not np.isnan(row).all() else np.nan for row in frames]), frames


def same_specials(got, want):
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want)) and not np.isneginf(got).any()


def max_diff(got, want):
    f = np.isfinite(want)
    return float(np.abs(got[f] - want[f]).max()) if f.any() else 0.0


# (S, C, L, win, hop, dead): W = 0 | one window, one row | odd sizes, tail dropped, K = 3 | overlap, K = 5 | gaps, K = 4 |
# W = 3000 > threads, not a power of two, K = 2998 | W = 15, K = 13 | a source whose reference is silent throughout: K = 0
CASES = [(2, 2, 99, 100, 100, False), (1, 1, 100, 100, 100, False), (2, 2, 3 * 1001 + 5, 1001, 1001, False), (3, 2, 4096, 1024, 512, False),
         (2, 2, 1350, 100, 250, False), (2, 2, 8 * 3000, 8, 8, False), (2, 2, 4096 + 3, 512, 256, False), (3, 2, 4096, 1024, 512, True)]


@pytest.mark.parametrize("S,C,L,win,hop,dead", CASES)
def test_frame_sdr_against_fp64(S, C, L, win, hop, dead):
    from fqss_amd import kernels as K
    from fqss_amd.process import calc_frame_sdr
    rng = np.random.default_rng(L + win)
    ref = rng.standard_normal((S, C, L)).astype(np.float32)
    est = (ref + 0.1 * rng.standard_normal((S, C, L))).astype(np.float32)
    W = (L - win) // hop + 1 if L >= win else 0
    span = lambda w: slice(w * hop, w * hop + win)
    if W >= 4:
        ref[0, :, span(0)] = 0.0                    # a silent reference: NaN in every source's row
        est[S - 1, :, span(1)] = 0.0                # a silent estimate
        ref[0, 0, span(3)] = 0.0                    # one channel of two is silent: the window stays valid
        est[0, :, span(2)] = ref[0, :, span(2)]     # den = 0: +inf
    if dead:
        ref[1] = 0.0
    want_med, want = frame_sdr_np(ref, est, win, hop)
    dense_r, dense_e = torch.from_numpy(ref).cuda(), torch.from_numpy(est).cuda()
    view_r, view_e = (torch.zeros(S, C, L + 6, device="cuda")[..., 1:L + 1] for _ in range(2))       # ld > L, a base one sample in
    view_r.copy_(dense_r), view_e.copy_(dense_e)
    med, frames = calc_frame_sdr(dense_r, dense_e, win, hop)
    med_v, frames_v = K.frame_sdr(view_e, view_r, win, hop)
    assert frames.shape == (S, W) and frames.dtype == torch.float64 and med.shape == (S,)
    # the 16-byte form (dense rows when L, hop are multiples of 4) and the one-sample form (the view) add in one order
    assert frames.view(torch.int64).equal(frames_v.view(torch.int64)) and med.view(torch.int64).equal(med_v.view(torch.int64))
    med, frames = med.cpu().numpy(), frames.cpu().numpy()
    K_valid = int((~np.isnan(want[0])).sum()) if W else 0
    print(f"W {W} K {K_valid}: max |diff| frames {max_diff(frames, want):.3g} dB, med {max_diff(med, want_med):.3g} dB; med {med}")
    assert same_specials(frames, want) and same_specials(med, want_med)
    assert max_diff(frames, want) <= 1e-9 and max_diff(med, want_med) <= 1e-9
    if W >= 4 and not dead:
        assert np.isnan(frames[:, :2]).all() and np.isposinf(frames[0, 2]) and np.isfinite(frames[:, 3]).all()
    if W == 0 or dead:
        assert np.isnan(med).all()


@pytest.mark.parametrize("what,match", [("win", "win >= 1"), ("hop", "hop >= 1"), ("windows", "FQSS_FSDR_MAX_WINDOWS"),
                                        ("workspace", "workspace shorter"), ("shape", "one shape")])
def test_frame_sdr_refusals(what, match):
    from fqss_amd import _lib
    from fqss_amd import kernels as K
    x = torch.randn(2, 2, K.FSDR_MAX_WINDOWS + 1, device="cuda")
    with pytest.raises((_lib.FqssError, AssertionError), match=match):
        if what == "workspace":
            med, n = torch.full((2,), 7.0, device="cuda", dtype=torch.float64), _lib.query("fqss_frame_sdr_ws_doubles", 2, 2, 64, 8, 8)
            ws = torch.empty(n, device="cuda", dtype=torch.float64)
            try:
                _lib.call("fqss_frame_sdr", x.data_ptr(), x.data_ptr(), ws.data_ptr(), n - 1, None, med.data_ptr(), 2, 2, 64, 8, 8,
                          x.shape[-1], x.shape[-1], None)
            finally:
                assert n == 3 * 2 * 8 and med.tolist() == [7.0, 7.0], "nothing is launched"
        else:
            K.frame_sdr(x[:, :1] if what == "shape" else x, x, 0 if what == "win" else 1, 0 if what == "hop" else 1)


class Stub(torch.nn.Module):
    """[B, C, T] -> [B, 3, C, T]: per-source scaled and shifted copies, element by element (the batch size cannot change a bit)"""
    n_srcs, n_splitter, audio_channels, sources = 3, 1, 2, ["drums", "bass", "vocals"]

    def forward(self, x):
        return torch.stack([x * 0.5 + 0.25, x * -1.5, x + 1.0], dim=1)


def test_val_musdbhq_frames(tmp_path, monkeypatch, capsys):
    import yaml
    from fqss_amd import kernels as K
    from fqss_amd import val
    from fqss_amd.process import model_infer
    rng, stub, meds = np.random.default_rng(11), Stub().cuda(), []
    for name in ("t0", "t1"):
        folder = tmp_path / "db" / name
        folder.mkdir(parents=True)
        pcm = {s: rng.integers(-9000, 9000, (8820, 2)).astype("<i2") for s in ["mixture"] + Stub.sources}      # 0.2 s: 4 windows of 2205
        for s, a in pcm.items():
            with wave.open(str(folder / (s + ".wav")), "wb") as w:
                w.setnchannels(2), w.setsampwidth(2), w.setframerate(44100), w.writeframes(a.tobytes())
        mix = torch.from_numpy(pcm["mixture"].T.astype(np.float32) / 32768.0).cuda()
        st = K.track_stats(mix)
        sep = model_infer(stub, (mix - st[0]) / st[1], segment=4000) * st[1] + st[0]
        refs = np.stack([pcm[s].T.astype(np.float32) / 32768.0 for s in Stub.sources])
        meds.append(frame_sdr_np(refs, sep.cpu().numpy(), 2205, 2205)[0])
    want = np.nanmedian(np.stack(meds, axis=1), axis=1)
    cfg = dict(model_cfg=dict(name="stub", quantization=dict(qat=True)), dataset_cfg=dict(name="musdbhq"),
               testing_cfg=dict(test_dir=str(tmp_path / "db"), frame_sdr=True, frame_win_s=0.05, segment_samples=4000, overlap=0.25))
    monkeypatch.setattr(val, "create_pretrained_model", lambda model_cfg: Stub())
    monkeypatch.setattr(sys, "argv", ["val"])
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    got = val.val(["-y", str(tmp_path / "cfg.yaml")])
    print(got, want)
    assert len(got) == 4 and np.abs(np.array(got[1:]) - want).max() <= 1e-9 and abs(got[0] - want.mean()) <= 1e-9
    assert "SDR={:0.2f},SDR_DRUMS={:0.2f},SDR_BASS={:0.2f},SDR_VOCALS={:0.2f}".format(*got) in capsys.readouterr().out
    cfg["testing_cfg"]["chunk_batch"] = 2
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    assert val.val(["-y", str(tmp_path / "cfg.yaml")]) == got             # chunk batches: the same numbers to the last bit
