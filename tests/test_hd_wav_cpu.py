"""Host side of the htdemucs env's WAV dataset (fqss_amd/train_env/htdemucs_musdbhq/wav_dataset.py) and of `kernels.hd_augment_mix`:
which files, which window, the int16 block, the metadata cache, the augmentation table and every refusal.  No kernel is launched;
every WAV tree is written into tmp_path with numpy + `wave`."""
import json
import os
import wave

import numpy as np
import pytest
import torch

SR = 8000
SRC = ["a", "b"]


def write_wav(path, data, rate=SR, width=2):
    """data: int array [frames, channels]"""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(data.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(data).astype({1: "u1", 2: "<i2", 4: "<i4"}[width]).tobytes())


def make_track(folder, L, C=2, seed=0, sources=SRC, mixture=False, amp=20000):
    rng = np.random.default_rng(seed)
    stems = [rng.integers(-amp, amp, size=(L, C), dtype=np.int64).astype(np.int16) for _ in sources]
    for name, x in zip(sources, stems):
        write_wav(os.path.join(folder, name + ".wav"), x)
    if mixture:
        write_wav(os.path.join(folder, "mixture.wav"), rng.integers(-amp, amp, size=(L, C), dtype=np.int64).astype(np.int16))
    return np.stack(stems)            # [S, L, C] int16


def dataset(dirs, **kw):
    from fqss_amd.train_env.htdemucs_musdbhq.wav_dataset import WavStems
    args = dict(sources=SRC, samplerate=SR, channels=2, segment=0.05, shift=0.0125, train=True, device="cpu")   # seg 400, stride 100
    args.update(kw)
    return WavStems(dirs, **args)


def test_example_counts_and_window_starts(tmp_path):
    seg, stride = 400, 100
    lengths = [seg - 7, seg, seg + 1, seg + 3 * stride - 1]
    dirs = [str(tmp_path / f"t{i}") for i in range(len(lengths))]
    for i, (d, L) in enumerate(zip(dirs, lengths)):
        make_track(d, L, seed=i)
    ds = dataset(dirs)
    assert (ds.T_in, ds.T_out, ds.stride) == (seg, seg - stride, stride)
    want = [(0, 0), (1, 0), (2, 0), (2, stride), (3, 0), (3, stride), (3, 2 * stride), (3, 3 * stride)]     # 1, 1, 2, 4 examples
    assert len(ds) == len(want) and [ds.example(i) for i in range(len(ds))] == want
    with pytest.raises(IndexError):
        ds.example(len(ds))
    # shift 0 / absent: hopped by seg, nothing cropped
    ds0 = dataset(dirs, shift=0)
    assert (ds0.T_in, ds0.T_out) == (seg, seg)
    assert [ds0.example(i) for i in range(len(ds0))] == [(0, 0), (1, 0), (2, 0), (2, seg), (3, 0), (3, seg)]
    # validation: consecutive windows of the training length
    dv = dataset(dirs, train=False)
    assert (dv.T_in, dv.T_out) == (seg - stride, seg - stride)
    assert [dv.example(i) for i in range(len(dv))] == [(0, 0), (0, 300), (1, 0), (1, 300), (2, 0), (2, 300), (3, 0), (3, 300), (3, 600)]
    assert len(dataset(dirs, train=False, max_examples=4)) == 4


def test_int16_passthrough_and_zero_padding(tmp_path):
    from fqss_amd.train_env.htdemucs_musdbhq.wav_dataset import SeededBatch
    L = 400 + 2 * 100 - 1
    d = str(tmp_path / "t")
    stems = make_track(d, L, amp=32768)
    stems[0, 5, 0], stems[1, 6, 1] = -32768, 32767
    for name, x in zip(SRC, stems):
        write_wav(os.path.join(d, name + ".wav"), x)
    ds = dataset([d])
    assert len(ds) == 3
    stage = torch.full((ds.stage_elems(3),), float("nan"))
    pcm, table, mean, std = ds.host_batch(SeededBatch([2, 0, 1], 5), stage)
    assert pcm.dtype == torch.int16 and pcm.shape == (3, 2, 400, 2) and mean is None and std is None
    assert pcm.data_ptr() == stage.data_ptr()                                     # the int16 block is a view of the staging buffer
    got = pcm.numpy()
    assert np.array_equal(got[1], stems[:, :400]) and got[1, 0, 5, 0] == -32768 and got[1, 1, 6, 1] == 32767
    assert np.array_equal(got[2], stems[:, 100:500])
    assert np.array_equal(got[0, :, :L - 200], stems[:, 200:]) and not got[0, :, L - 200:].any()      # zeros behind the track
    assert table.off.shape == (3, 2) and int(table.off.max()) < 100
    with pytest.raises(ValueError, match="seed"):
        ds.host_batch([0])                                                        # a training batch without its position's seed
    # a track shorter than the window: one example, padded
    short = str(tmp_path / "s")
    st = make_track(short, 123, seed=3)
    pcm, table, _, _ = dataset([short], train=False).host_batch([0])
    assert np.array_equal(pcm.numpy()[0, :, :123], st) and not pcm.numpy()[0, :, 123:].any()
    assert torch.equal(table.src_b, torch.zeros(1, 2, dtype=torch.int64)) and torch.equal(table.gain, torch.ones(1, 2))


@pytest.mark.parametrize("mixture", [False, True])
def test_track_mean_std_against_numpy_fp64(tmp_path, monkeypatch, mixture):
    from fqss_amd.train_env.htdemucs_musdbhq import wav_dataset as W
    monkeypatch.setattr(W, "_STAT_BLOCK", 1000)               # several blocks and a ragged last one
    d = str(tmp_path / "t")
    L = 4321
    stems = make_track(d, L, mixture=mixture, seed=7)
    if mixture:
        with wave.open(os.path.join(d, "mixture.wav"), "rb") as w:
            x = np.frombuffer(w.readframes(L), dtype="<i2").reshape(L, 2).astype(np.float64) / 32768.0
    else:
        x = stems.astype(np.float64).sum(axis=0) / 32768.0
    mono = x.mean(axis=1)
    ds = dataset([d], normalize=True)
    assert abs(ds.mean[0] - mono.mean()) <= 1e-12 * abs(mono.mean()) + 1e-18
    assert abs(ds.std[0] - mono.std(ddof=1)) <= 1e-12 * mono.std(ddof=1)
    _, _, mean, std = ds.host_batch(W.SeededBatch([0, 1], 1))
    assert mean.dtype == torch.float32 and torch.equal(mean, torch.tensor([mono.mean()] * 2, dtype=torch.float64).float())
    assert torch.equal(std, torch.tensor([mono.std(ddof=1)] * 2, dtype=torch.float64).float())
    if mixture:
        other = stems.astype(np.float64).sum(axis=0).mean(axis=1) / 32768.0
        assert abs(ds.std[0] - other.std(ddof=1)) > 1e-3                          # mixture.wav was used, not the stems' sum


def test_metadata_cache_is_reused(tmp_path, monkeypatch):
    from fqss_amd.train_env.htdemucs_musdbhq import wav_dataset as W
    dirs = [str(tmp_path / "tracks" / f"t{i}") for i in range(3)]
    for i, d in enumerate(dirs):
        make_track(d, 700 + i, seed=i)
    cache = str(tmp_path / "work" / W.CACHE_NAME)
    opened = []
    real = wave.open
    monkeypatch.setattr(W.wave, "open", lambda f, mode=None: (opened.append(f) if mode == "rb" else None, real(f, mode))[1])
    a = dataset(dirs, normalize=True, cache_file=cache)
    assert len(opened) == 6 and os.path.exists(cache)
    assert set(json.load(open(cache))) == {os.path.abspath(d) for d in dirs}
    del opened[:]
    b = dataset(dirs, normalize=True, cache_file=cache)
    assert opened == []                                                            # the second construction reads no stem
    assert (a.length, a.mean, a.std) == (b.length, b.mean, b.std)
    # a stem that changed (size / mtime) is read again, the others are not
    make_track(dirs[1], 650, seed=9)
    c = dataset(dirs, normalize=True, cache_file=cache)
    assert len(opened) == 2 and all(dirs[1] in f for f in opened) and c.length == [700, 650, 702] and c.std[1] != a.std[1]


def test_file_refusals_name_the_file(tmp_path):
    def fresh(name):
        d = str(tmp_path / name)
        make_track(d, 900)
        return d, os.path.join(d, "b.wav")

    x = np.zeros((900, 2), dtype=np.int16)
    d, f = fresh("rate")
    write_wav(f, x, rate=SR * 2)
    with pytest.raises(ValueError, match=r"rate.b\.wav.*sample rate 16000"):
        dataset([d])
    d, f = fresh("width")
    write_wav(f, x.astype(np.int32), width=4)
    with pytest.raises(ValueError, match=r"width.b\.wav.*32-bit"):
        dataset([d])
    d, f = fresh("chan")
    write_wav(f, x[:, :1])
    with pytest.raises(ValueError, match=r"chan.b\.wav.*1 channels"):
        dataset([d])
    d, f = fresh("missing")
    os.remove(f)
    with pytest.raises(FileNotFoundError, match=r"missing.b\.wav"):
        dataset([d])
    d, f = fresh("length")
    write_wav(f, x[:899])
    with pytest.raises(ValueError, match=r"length.b\.wav.*899 frames"):
        dataset([d])
    d, f = fresh("junk")
    open(f, "wb").write(b"not a wav file at all")
    with pytest.raises(ValueError, match=r"junk.b\.wav"):
        dataset([d])
    d, f = fresh("mixlen")
    write_wav(os.path.join(d, "mixture.wav"), x[:10])
    with pytest.raises(ValueError, match=r"mixlen.mixture\.wav.*10 frames"):
        dataset([d], normalize=True)
    d = str(tmp_path / "silent")
    for s in SRC:
        write_wav(os.path.join(d, s + ".wav"), x)
    with pytest.raises(ValueError, match=r"silent.*standard deviation"):
        dataset([d], normalize=True)
    dataset([d])                                                                  # ... which only normalisation minds


def test_layouts(tmp_path):
    from fqss_amd.train_env.htdemucs_musdbhq import wav_dataset as W
    root = tmp_path / "custom"
    for part, names in (("train", ["x", "y"]), ("valid", ["z"])):
        for n in names:
            make_track(str(root / part / n), 500)
    tr, va = W.split_tracks({"wav": str(root)})
    assert [os.path.basename(p) for p in tr] == ["x", "y"] and [os.path.basename(p) for p in va] == ["z"]
    assert W.configured({"wav": str(root)}) and not W.configured({"name": "synthetic", "wav": str(root)}) and not W.configured({"musdb": "/m"})
    mus = {"musdb": str(root), "use_musdb": True}
    assert W.configured(mus)
    with pytest.raises(ValueError, match="valid_tracks"):
        W.split_tracks(mus)
    tr, va = W.split_tracks(dict(mus, valid_tracks=["y"]))
    assert [os.path.basename(p) for p in tr] == ["x"] and [os.path.basename(p) for p in va] == ["y"]
    with pytest.raises(FileNotFoundError, match="nope"):
        W.split_tracks(dict(mus, valid_tracks=["nope"]))
    with pytest.raises(NotImplementedError, match="wav2"):
        W.split_tracks({"wav": str(root), "wav2": "/x"})
    conf = {"work_dir": str(tmp_path / "w"), "dset": dict(mus, valid_tracks=["y"], sources=SRC, samplerate=SR, channels=2, segment=0.05,
                                                           shift=0.0125, normalize=True, valid_samples=1),
            "augment": {"flip": True}}
    train, valid = W.build_datasets(conf, device="cpu")
    assert train.train and not valid.train and len(valid) == 1 and train.augment == {"flip": True}
    assert os.path.exists(os.path.join(conf["work_dir"], W.CACHE_NAME))


CFG = {"shift_same": False, "flip": True, "repitch": {"proba": 0, "max_tempo": 12}, "remix": {"proba": 1, "group_size": 4},
       "scale": {"proba": 1, "min": 0.25, "max": 1.25}}


def _draw(seed, B=8, S=4, C=2, shift=441, **over):
    from fqss_amd.train_env.htdemucs_musdbhq.wav_dataset import draw_augment
    return draw_augment(B, S, C, shift, dict(CFG, **over), torch.Generator().manual_seed(seed))


def test_draw_augment_is_a_function_of_the_seed():
    a, b, c = _draw(11), _draw(11), _draw(12)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not all(torch.equal(x, y) for x, y in zip(a, c))
    assert a.src_b.dtype == a.off.dtype == a.flip.dtype == torch.int64 and a.gain.dtype == torch.float32
    assert all(t.shape == (8, 4) for t in a)


def test_draw_augment_remix_permutes_inside_groups():
    moved = 0
    for seed in range(20):
        t = _draw(seed)
        for s in range(4):
            for g in range(2):
                assert sorted(t.src_b[4 * g:4 * g + 4, s].tolist()) == list(range(4 * g, 4 * g + 4))      # a permutation; no item crosses a group
        moved += int((t.src_b != torch.arange(8)[:, None]).sum())
        whole = _draw(seed, remix={"proba": 1, "group_size": None})
        assert all(sorted(whole.src_b[:, s].tolist()) == list(range(8)) for s in range(4))
        # remix moves whole augmented rows: the row of output (b, s) is the one drawn for (src_b[b, s], s)
        base = _draw(seed, remix={"proba": 0})
        for f in ("off", "flip", "gain"):
            assert torch.equal(getattr(t, f), getattr(base, f).gather(0, t.src_b)), f
    assert moved > 200
    with pytest.raises(ValueError, match="divisible"):
        _draw(0, B=6)


def test_draw_augment_ranges():
    signs, flips, offs = set(), set(), set()
    for seed in range(20):
        t = _draw(seed)
        assert int(t.off.min()) >= 0 and int(t.off.max()) < 441
        assert float(t.gain.abs().min()) >= 0.25 and float(t.gain.abs().max()) <= 1.25
        assert set(t.flip.unique().tolist()) <= {0, 1}
        signs |= set(torch.sign(t.gain).unique().tolist())
        flips |= set(t.flip.unique().tolist())
        offs |= set(t.off.unique().tolist())
        same = _draw(seed, shift_same=True, remix={"proba": 0})
        assert bool((same.off == same.off[:, :1]).all())                           # one offset per item
        assert not bool((t.off == t.off[:, :1]).all())
    assert signs == {-1.0, 1.0} and flips == {0, 1} and len(offs) > 200 and max(offs) > 400
    t = _draw(3, shift=0)
    assert not t.off.any()
    t = _draw(3, C=1)
    assert not t.flip.any() and set(torch.sign(t.gain).unique().tolist()) == {-1.0, 1.0}      # mono: no swap, the sign stays
    t = _draw(3, flip=False)
    assert not t.flip.any() and float(t.gain.min()) >= 0.25
    t = _draw(3, scale={"proba": 0, "min": 0.25, "max": 1.25}, remix={"proba": 0, "group_size": 4})
    assert set(t.gain.abs().unique().tolist()) == {1.0} and torch.equal(t.src_b, torch.arange(8)[:, None].expand(8, 4))
    from fqss_amd.train_env.htdemucs_musdbhq.wav_dataset import draw_augment, identity_table
    t = draw_augment(3, 2, 2, 0, None, torch.Generator().manual_seed(0))         # no augment block at all: the identity
    assert all(torch.equal(x, y) for x, y in zip(t, identity_table(3, 2)))


def test_repitch_and_group_size_are_refused_before_anything_is_read(tmp_path):
    from fqss_amd.train_env.htdemucs_musdbhq import wav_dataset as W
    with pytest.raises(NotImplementedError, match=r"augment\.repitch\.proba"):
        _draw(0, repitch={"proba": 0.2, "max_tempo": 12})
    with pytest.raises(NotImplementedError, match=r"augment\.repitch\.proba"):
        W.check_augment_cfg({"repitch": {"proba": 0.2}})
    with pytest.raises(NotImplementedError, match=r"augment\.repitch\.proba"):
        dataset([str(tmp_path / "never_read")], augment={"repitch": {"proba": 0.2}})
    with pytest.raises(ValueError, match="group_size 4"):
        W.check_augment_cfg(CFG, 6)
    W.check_augment_cfg(CFG, 8)
    W.check_augment_cfg(dict(CFG, remix={"proba": 0, "group_size": 4}), 6)


def test_shipped_wav_config_parses_and_is_a_wav_configuration():
    import yaml
    from fqss_amd.train_env.htdemucs_musdbhq import wav_dataset as W
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    conf = yaml.safe_load(open(os.path.join(root, "configs", "htdemucs_wav.yaml")))
    assert W.configured(conf["dset"]) and conf["augment"]["repitch"]["proba"] == 0
    W.check_augment_cfg(conf["augment"], conf["batch_size"] // 8)
    with pytest.raises(ValueError, match="valid_tracks"):
        W.split_tracks(conf["dset"])
    synth = yaml.safe_load(open(os.path.join(root, "configs", "htdemucs_synthetic.yaml")))
    assert not W.configured(synth["dset"])


def test_wrapper_range_checks_raise_before_any_library_call(monkeypatch):
    """every kind of bad table is a ValueError raised on the host; nothing is uploaded, nothing is launched (no device here)"""
    from fqss_amd import _lib, kernels as K
    from fqss_amd.train_env.htdemucs_musdbhq.wav_dataset import identity_table
    called = []
    monkeypatch.setattr(_lib, "call", lambda *a: called.append(a))
    B, S, T_in, T_out = 3, 2, 50, 40
    pcm = torch.zeros(B, S, T_in, 2, dtype=torch.int16)
    mean, std = torch.zeros(B), torch.ones(B)

    def run(pcm=pcm, T_out=T_out, mean=mean, std=std, **over):
        t = identity_table(B, S)._replace(**over)
        return K.hd_augment_mix(pcm, T_out, t.src_b, t.off, t.flip, t.gain, mean, std)

    def table(v, dtype=torch.int64):
        t = torch.zeros(B, S, dtype=dtype)
        t[1, 1] = v
        return t

    bad = [dict(src_b=table(B)), dict(src_b=table(-1)), dict(off=table(T_in - T_out + 1)), dict(off=table(-1)), dict(flip=table(2)),
           dict(flip=table(-1)), dict(gain=table(float("nan"), torch.float32)), dict(gain=table(float("inf"), torch.float32)),
           dict(gain=torch.ones(B, S, dtype=torch.float64)), dict(std=torch.tensor([1.0, 0.0, 1.0])), dict(std=torch.tensor([1.0, -1.0, 1.0])),
           dict(std=torch.tensor([1.0, float("nan"), 1.0])), dict(mean=torch.tensor([0.0, float("inf"), 0.0])), dict(std=None),
           dict(mean=torch.zeros(B + 1)), dict(off=torch.zeros(B, S + 1, dtype=torch.int64)), dict(src_b=torch.zeros(B, S)),
           dict(T_out=T_in + 1), dict(T_out=0), dict(src_b=None), dict(off=None), dict(flip=None), dict(gain=None), dict(pcm=torch.zeros(B, 9, T_in, 2, dtype=torch.int16)),
           dict(pcm=torch.zeros(B, S, T_in, 3, dtype=torch.int16)), dict(pcm=torch.zeros(B, S, T_in, 2))]
    for kw in bad:
        with pytest.raises(ValueError):
            run(**kw)
    with pytest.raises(ValueError, match="int32"):                                # an offset the int32 table could not carry
        K.check_augment_table(1, 1, 1, 1 << 31, 8, *identity_table(1, 1))
    run_ok = dict(off=table(T_in - T_out))
    with pytest.raises(_lib.FqssError, match="no CPU fallback"):                   # a good table gets as far as the device check
        run(**run_ok)
    assert called == []
