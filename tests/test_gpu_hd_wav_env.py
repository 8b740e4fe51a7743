"""The htdemucs env on folders of WAV stems (train_env/htdemucs_musdbhq/{train,wav_dataset}.py): `main()` on a generated tree -- 5
training and 2 validation tracks of 0.3 to 0.5 s, 44.1 kHz stereo, 2 sources -- with the tiny HTDemucs of test_htdemucs_env_trains;
the data path is a pure function of (seed, epoch, batch index), across a resume too, and is the statement of include/fqss.h applied
to the files."""
import os
import sys
import wave

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR, SRC = 44100, ["a", "b"]


def write_tree(root):
    rng = np.random.default_rng(0)
    for part, n in (("train", 5), ("valid", 2)):
        for i in range(n):
            L = int(rng.integers(int(0.3 * SR), int(0.5 * SR)))
            for s in SRC:
                x = (rng.standard_normal((L, 2)) * 3000 * (1 + i)).clip(-32768, 32767).astype("<i2")
                path = os.path.join(root, part, f"track{i}", s + ".wav")
                os.makedirs(os.path.dirname(path), exist_ok=True)
                with wave.open(path, "wb") as w:
                    w.setnchannels(2)
                    w.setsampwidth(2)
                    w.setframerate(SR)
                    w.writeframes(x.tobytes())


def make_conf(tmp, tree, **over):
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "htdemucs_wav.yaml")))
    conf["work_dir"] = str(tmp / "run")
    conf["dset"].update(wav=str(tree), use_musdb=False, segment=0.06, shift=0.01, sources=SRC, valid_steps=2)
    conf["augment"]["remix"]["group_size"] = 2
    conf.update(epochs=2, batch_size=2, weights=[1.0, 1.0], max_batches=28)
    conf["htdemucs"] = dict(nfft=2048, channels=8, bottom_channels=16, t_layers=3, t_heads=2)
    conf.update(over)
    yml = tmp / f"cfg{len(os.listdir(tmp))}.yaml"
    yml.write_text(yaml.safe_dump(conf))
    return conf, yml


def run_main(yml, *extra):
    """main() with the reference's command line; returns (history, the training batches the reader made, in order)"""
    from fqss_amd.train_env.htdemucs_musdbhq import train as T
    from fqss_amd.train_env.htdemucs_musdbhq.wav_dataset import WavStems
    seen, real, argv = [], WavStems.batch, sys.argv

    def batch(self, indices, stage=None):
        mix, src = real(self, indices, stage)
        if self.train:
            seen.append((list(indices), indices.seed, mix.clone(), src.clone()))
        return mix, src

    WavStems.batch, sys.argv = batch, ["train.py", "+device=cuda", f"+yml_path={yml}", "optim.lr=0.0002", *extra]
    try:
        hist = T.main()
    finally:
        WavStems.batch, sys.argv = real, argv
    torch.cuda.synchronize()
    return hist, seen


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("hd_wav")
    tree = tmp / "tree"
    write_tree(str(tree))
    conf, yml = make_conf(tmp, tree)
    hist, seen = run_main(yml)
    return dict(tmp=tmp, tree=tree, conf=conf, hist=hist, seen=seen)


def test_wav_env_trains(trained):
    from fqss_amd.train_env.htdemucs_musdbhq.wav_dataset import CACHE_NAME
    hist, conf = trained["hist"], trained["conf"]
    assert len(hist) == 2
    for h in hist:
        assert np.isfinite(h["train"]["loss"]) and np.isfinite(h["valid"]["loss"])
        assert h["train"]["loader_wait_s"] >= 0.0 and h["valid"]["loader_wait_s"] >= 0.0
    assert [h["train"]["launch"] for h in hist] == ["eager", "hipGraph replay"]          # the observer phase ended inside the run
    assert len(trained["seen"]) == 2 * 28
    pkg = torch.load(os.path.join(conf["work_dir"], "best.th"))
    assert set(pkg) == {"state", "kwargs", "history"} and pkg["kwargs"]["nfft"] == 2048
    assert "decoder.3.conv_tr.residual_error_block.weight_fake_quantize_dec.min_range" in pkg["state"]
    assert os.path.exists(os.path.join(conf["work_dir"], CACHE_NAME))
    assert os.path.exists(os.path.join(conf["work_dir"], "checkpoint.pth"))


def statement(pcm, T_out, src_b, off, flip, gain, mean, std):
    """include/fqss.h, fqss_hd_augment_mix, in torch CPU fp32 ops, one per line"""
    B, S, T_in, C = pcm.shape
    sources = torch.empty(B, S, C, T_out, dtype=torch.float32)
    for b in range(B):
        for s in range(S):
            bs, o = int(src_b[b, s]), int(off[b, s])
            for c in range(C):
                v = pcm[bs, s, o:o + T_out, 1 - c if int(flip[b, s]) else c].to(torch.float32)
                v = v * torch.tensor(2.0 ** -15, dtype=torch.float32)
                v = v - mean[bs]
                v = v / std[bs]
                v = v * gain[b, s]
                sources[b, s, c] = v
    mix = sources[:, 0].clone()
    for s in range(1, S):
        mix = mix + sources[:, s]
    return mix, sources


def test_first_batch_is_the_statement_applied_to_the_files(trained):
    """the batch the solver saw at (epoch 0, index 0): the files' windows read here with `wave`, the tracks' fp64 mean / std, the table
    `draw_augment` gives for that position's seed, and the statement -- torch.equal"""
    from fqss_amd.train_env.htdemucs_musdbhq.wav_dataset import batch_seed, draw_augment
    conf = trained["conf"]
    indices, seed, mix, src = trained["seen"][0]
    assert seed == batch_seed(conf["seed"], 0, 0, 0, 1) and len(indices) == 2
    seg, stride = int(SR * 0.06), int(SR * 0.01)
    tracks = []
    for name in sorted(os.listdir(trained["tree"] / "train")):
        stems = []
        for s in SRC:
            with wave.open(str(trained["tree"] / "train" / name / (s + ".wav")), "rb") as w:
                stems.append(np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").reshape(-1, 2))
        tracks.append(np.stack(stems))                                               # [S, L, C]
    first = np.cumsum([0] + [-(-(t.shape[1] - seg) // stride) + 1 for t in tracks])
    pcm = np.zeros((2, 2, seg, 2), dtype=np.int16)
    mean, std = [], []
    for b, i in enumerate(indices):
        k = int(np.searchsorted(first, i, side="right")) - 1
        win = tracks[k][:, (i - first[k]) * stride:][:, :seg]
        pcm[b, :, :win.shape[1]] = win
        mono = (tracks[k].astype(np.float64).sum(axis=0) / 32768.0).mean(axis=1)
        mean.append(mono.mean())
        std.append(mono.std(ddof=1))
    f32 = lambda v: torch.tensor(v, dtype=torch.float64).to(torch.float32)
    table = draw_augment(2, 2, 2, stride, conf["augment"], torch.Generator().manual_seed(seed))
    assert int(table.off.max()) > 0 and float(table.gain.abs().min()) < 1.25
    want_mix, want_src = statement(torch.from_numpy(pcm), seg - stride, *table, f32(mean), f32(std))
    assert src.shape == (2, 2, 2, seg - stride) and torch.equal(src.cpu(), want_src)
    assert torch.equal(mix.cpu(), want_mix)


def test_resumed_run_reads_the_batches_of_the_uninterrupted_run(trained, tmp_path):
    """1 epoch, then `resume=auto` to epoch 2: the batches of epoch 2 equal those of an uninterrupted 2-epoch run (indices, seeds,
    mixtures and stems, torch.equal).  Model bits are not compared: the HTDemucs step is not bit-reproducible by default."""
    _, yml = make_conf(tmp_path, trained["tree"], max_batches=3, work_dir=str(tmp_path / "whole"))
    hist, want = run_main(yml)
    assert len(hist) == 2 and len(want) == 6
    conf, yml1 = make_conf(tmp_path, trained["tree"], max_batches=3, epochs=1, work_dir=str(tmp_path / "split"))
    hist, first = run_main(yml1)
    assert len(hist) == 1 and len(first) == 3
    _, yml2 = make_conf(tmp_path, trained["tree"], max_batches=3, epochs=2, work_dir=str(tmp_path / "split"))
    hist, second = run_main(yml2, "resume=auto")
    assert len(hist) == 2 and len(second) == 3
    for got, ref in zip(first + second, want):
        assert got[0] == ref[0] and got[1] == ref[1]
        assert torch.equal(got[2], ref[2]) and torch.equal(got[3], ref[3])
    assert [w[0] for w in want[:3]] != [w[0] for w in want[3:]]                      # the second epoch is another order
