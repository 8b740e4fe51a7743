#!/usr/bin/env python3
"""`val.py -y cfg.yaml` (reference: val.py:17-25, 59-92, 184-226): load the quantized model, run `model_infer` over the evaluation
set and report SI-SDR, its improvement over the unprocessed mixture, and SDR (fqss_sdr: torchmetrics' SignalDistortionRatio
restated).  `dataset_cfg.name: librimix` walks `testing_cfg.test_dir` as val.py:28-92 does (mix_clean | mix_both | mix_single,
s1..s3; whole utterances, resampled on the device); `synthetic` evaluates seeded two-speaker mixtures.  STOI (pystoi: third party,
absent) is printed as nan unless `testing_cfg.stoi: true` asks for fqss_stoi, the restated definition, at the utterance's rate;
`testing_cfg.stoi_extended: true` beside it puts the extended measure (ESTOI, fqss_stoi_x) into the same slot.
`testing_cfg.bss_eval: true` (librimix) appends `,SIR=..,SAR=..` -- BSS-eval's interference and artefact ratios, fqss_bss_eval, the
definition of mir_eval / fast_bss_eval restated -- to the result and progress lines; without the key the lines are what they were.
`dataset_cfg.name: musdbhq` with `testing_cfg.NSDR: true` is the reference's `val_musdbhq_NSDR` (val.py:95-131) over folders of WAV
stems (`val_musdbhq_nsdr` below: the `musdb` package is not needed for it); without NSDR the branch needs `museval` (absent): refused,
unless `testing_cfg.frame_sdr: true` asks for museval's SDR restated -- the median over one-second windows, fqss_frame_sdr
(`val_musdbhq_frames` below; SIR / SAR / ISR are not computed).
`val()` returns (SI-SDR, improvement), or the nSDR / SDR tuple of the musdbhq branch; the SDR and the STOI of the run are in the
printed result line."""
import argparse
import glob
import os

import torch
import yaml

from . import kernels as K
from .data import synth_batch
from .process import bss_eval, metric_evaluation, model_infer
from .quantization.qat.models.load_model import create_pretrained_model, enable_observer


def argument_handler():
    p = argparse.ArgumentParser()
    p.add_argument("--yml_path", "-y", type=str, required=True, help="YML configuration file")
    p.add_argument("--use_cpu", action="store_true", help="Use cpu")
    return p.parse_args()


SYNTHETIC_RATE = 8000      # the synthetic mixtures stand in for the 8 kHz configs


def val_synthetic(model, model_cfg, dataset_cfg, testing_cfg, device):
    n_srcs = model_cfg.get("n_src", 1)
    n, L = testing_cfg.get("n_items", 4), int(testing_cfg.get("length_samples", 32000))
    with_stoi, extended = bool(testing_cfg.get("stoi", False)), bool(testing_cfg.get("stoi_extended", False))
    sisdr = sisdr_imp = sdr = stoi = 0.0
    for i in range(n):
        mix, clean = synth_batch(1, L, seed=10_000 + i, device=device)
        mix_wav, clean_wavs = mix[0], clean[0]                         # [1, L], [S, L]
        wavs = model_infer(model, mix_wav, n_srcs=n_srcs, segment=testing_cfg.get("segment_samples", None),
                           overlap=testing_cfg.get("overlap", 0.25), device=device, target=clean_wavs)
        s, d, st = metric_evaluation(wavs, clean_wavs, sample_rate=SYNTHETIC_RATE, with_stoi=with_stoi, stoi_extended=extended)
        base = K.sisnr_matrix(clean_wavs, mix_wav.expand(n_srcs, -1).contiguous())
        sisdr += s
        sisdr_imp += s - torch.diagonal(base).mean().item()
        sdr += d
        stoi += st
    return sisdr / n, sisdr_imp / n, sdr / n, stoi / n


def read_librimix(folder, n_spks=1, noisy=False):
    """file lists of a LibriMix test folder (val.py:28-57)"""
    assert 1 <= n_spks <= 3, "Error: Up to 3 sources to seperate!"
    mix_dir = "mix_single" if n_spks == 1 else ("mix_both" if noisy else "mix_clean")
    mix_audio_files = sorted(glob.glob(os.path.join(folder, mix_dir, "*")))
    clean = [sorted(glob.glob(os.path.join(folder, f"s{i + 1}", "*"))) for i in range(n_spks)]
    assert all(len(c) == len(mix_audio_files) for c in clean) and len(mix_audio_files) > 0, "Dataset is missing files!"
    return mix_audio_files, clean


def val_librimix(model, model_cfg, dataset_cfg, testing_cfg, device):
    """val.py:59-92: per utterance read mixture + sources, resample, model_infer, SI-SDR, its improvement over the mixture, and SDR.  The
    reader thread has utterance i + 1 (WAV reads, upload, resampling) on the device while utterance i is separated."""
    from .loader import Prefetcher
    from .train_env.asteroid_librimix.librimix_dataset import read_wav
    n_srcs = model_cfg.get("n_src", 1)
    mix_files, clean_lists = read_librimix(testing_cfg["test_dir"], n_srcs, dataset_cfg["noisy"])
    limit = testing_cfg.get("n_items")
    n = len(mix_files) if limit is None else min(int(limit), len(mix_files))
    ratio = dataset_cfg.get("resample", 1)

    class _Utterances:                       # one item per batch: (mixture [1, 1, L'], sources [1, S, L'])
        def stage_elems(self, batch_size):
            return 0

        def batch(self, indices, stage=None):
            i = indices[0]
            clips = [read_wav(mix_files[i])] + [read_wav(lst[i]) for lst in clean_lists]
            L = min(len(c) for c in clips)
            import numpy as np
            x = torch.from_numpy(np.stack([c[:L] for c in clips])).to(device)
            if ratio != 1:
                fs = int(dataset_cfg.get("sample_rate", 16000))
                x = K.resample(x, fs, int(fs * ratio))
            return x[:1].unsqueeze(0), x[1:].unsqueeze(0)

    with_stoi, extended = bool(testing_cfg.get("stoi", False)), bool(testing_cfg.get("stoi_extended", False))
    rate = int(int(dataset_cfg.get("sample_rate", 16000)) * ratio)       # the utterance's rate after resampling (val.py:83 passes fs too)
    with_bss, bss = bool(testing_cfg.get("bss_eval", False)), None      # BSS-eval (SDR, SIR, SAR) summed on the device
    sisdr = sisdr_imp = sdr = stoi = 0.0
    for i, (mix, clean) in enumerate(Prefetcher(_Utterances(), [[k] for k in range(n)], device, depth=1)):
        mix_wav, clean_wavs = mix[0], clean[0]
        wavs = model_infer(model, mix_wav, n_srcs=n_srcs, segment=testing_cfg.get("segment_samples", None),
                           overlap=testing_cfg.get("overlap", 0.25), device=device, target=clean_wavs,
                           chunk_batch=testing_cfg.get("chunk_batch"))
        s, d, st = metric_evaluation(wavs, clean_wavs, sample_rate=rate, with_stoi=with_stoi, stoi_extended=extended)
        # val.py:86: the sources as estimates, the mixture as target; only its SI-SNR is used
        base, _, _ = metric_evaluation(clean_wavs, mix_wav.expand(n_srcs, -1).contiguous(), with_sdr=False)
        sisdr += s
        sisdr_imp += s - base
        sdr += d
        stoi += st
        if with_bss:      # one more launch sequence per utterance; read back only where a line is printed
            b = bss_eval(wavs, clean_wavs)
            bss = b if bss is None else bss + b
        if (i % 500 == 0 and i > 0) or i == 1:
            print("SI-SDR={:0.3f},SI-SDR-imp={:0.3f},SDR={:0.3f}".format(sisdr / (i + 1), sisdr_imp / (i + 1), sdr / (i + 1))
                  + (",SIR={:0.3f},SAR={:0.3f}".format(*(bss[1:] / (i + 1)).tolist()) if with_bss else ""))
    return sisdr / n, sisdr_imp / n, sdr / n, stoi / n, (bss[1:] / n).tolist() if with_bss else None


def _read_stereo_wav(path, rate, channels, device):
    """[channels, L] fp32 on the device, int16 / 32768 (exact): what musdb's `track.audio` holds, transposed"""
    import numpy as np
    from .train_env.htdemucs_musdbhq.wav_dataset import _open_checked
    w = _open_checked(path, rate, channels)
    try:
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").reshape(-1, channels)
    finally:
        w.close()
    return torch.from_numpy(pcm.copy()).to(device).t().contiguous().float().div_(32768.0)


def _musdbhq_tracks(model, testing_cfg, device):
    """the track walk that val_musdbhq_nsdr and val_musdbhq_frames share: per track, normalise the mixture by the mean / std of its
    channel mean (fqss_track_stats), separate it chunk by chunk, de-normalise, read the stems.  Tracks are the sub-folders of
    `<test_dir>/test` when that folder exists, else of `<test_dir>`; each holds mixture.wav and <source>.wav for every model.sources,
    16-bit PCM at `testing_cfg.samplerate` (44100) with the model's channel count.  `testing_cfg.chunk_batch: G` sends G chunks per
    forward with the normalisation inside the gather and the overlap-add (process.model_infer(chunk_batch=G, stats=...)); absent, the
    chunks go one by one and both are tensor operations.  Yields (j, number of tracks, refs [S, C, L], separations [S, C, L])."""
    from .train_env.htdemucs_musdbhq.wav_dataset import MIXTURE, _list_tracks
    root = testing_cfg["test_dir"]
    if os.path.isdir(os.path.join(root, "test")):
        root = os.path.join(root, "test")
    tracks = _list_tracks(root)
    if not tracks:
        raise FileNotFoundError(f"{root}: no track folders (each holds {MIXTURE}.wav and one WAV per source)")
    print("{} tracks under {}".format(len(tracks), root))
    sources = list(model.sources)
    rate, channels = int(testing_cfg.get("samplerate", 44100)), int(getattr(model, "audio_channels", 2))
    segment, overlap, G = testing_cfg.get("segment_samples", None), testing_cfg.get("overlap", 0.25), testing_cfg.get("chunk_batch")
    for j, name in enumerate(tracks):
        read = lambda stem: _read_stereo_wav(os.path.join(root, name, stem + ".wav"), rate, channels, device)
        mix = read(MIXTURE)
        stats = K.track_stats(mix)
        if segment and G is not None:
            separations = model_infer(model, mix, segment=segment, overlap=overlap, device=device, chunk_batch=G, stats=stats)
        else:
            separations = model_infer(model, (mix - stats[0]) / stats[1], segment=segment, overlap=overlap, device=device)
            separations = separations * stats[1] + stats[0]
        refs = torch.stack([read(src) for src in sources])
        if refs.shape != separations.shape:
            raise ValueError(f"{os.path.join(root, name)}: stems {tuple(refs.shape)}, separations {tuple(separations.shape)}")
        yield j, len(tracks), refs, separations


def _print_track(model, j, n_tracks, column):
    if j % 10 == 0:
        print("\n****** Track {}/{} ******".format(j + 1, n_tracks))
        for src, v in zip(model.sources, column):
            print("{}: SDR={:0.3f}".format(src, v))


def val_musdbhq_nsdr(model, testing_cfg, device):
    """val_musdbhq_NSDR of the reference (val.py:95-131) on the device: every source of every track of _musdbhq_tracks scored with
    calc_nsdr (fqss_nsdr: one launch sequence and one read-back per track).
    Prints the reference's progress lines; returns (mean over sources, per-source means..).
    Differences from the reference: it asserts exactly 50 tracks (the MUSDB18-HQ test set) -- here an empty folder raises and any
    other count is printed; the files are read by the `wave` module, not by `musdb` (parity with that reader is not pinned); mean and
    std are fp64 sums rounded once, not torch's fp32 reductions."""
    import numpy as np
    from .process import calc_nsdr
    sdrs = None
    for j, n_tracks, refs, separations in _musdbhq_tracks(model, testing_cfg, device):
        if sdrs is None:
            sdrs = np.zeros((refs.shape[0], n_tracks))
        sdrs[:, j] = calc_nsdr(refs, separations).tolist()          # the track's one read-back
        _print_track(model, j, n_tracks, sdrs[:, j])
    sdrs = np.mean(sdrs, axis=1)
    return (float(np.mean(sdrs)),) + tuple(float(v) for v in sdrs)


def val_musdbhq_frames(model, testing_cfg, device):
    """the SDR of the reference's val_musdbhq (val.py:134-181: museval.eval_mus_track per track, agg_frames_tracks_scores over them) on
    the device, SDR only: every track of _musdbhq_tracks scored with calc_frame_sdr (fqss_frame_sdr: two launches and one read-back per
    track) in windows of `testing_cfg.frame_win_s` seconds (1.0) every `testing_cfg.frame_hop_s` seconds (the window), each
    int(seconds * samplerate) samples; per source the nanmedian over the tracks' medians, then the mean over sources.
    Returns (mean over sources, per-source values..).  museval is a third-party package that is absent: the window SDR and the
    silence rule are restated in include/fqss.h and parity with the package is not pinned; its SIR / SAR / ISR are not computed."""
    import warnings
    import numpy as np
    from .process import calc_frame_sdr
    rate = int(testing_cfg.get("samplerate", 44100))
    win_s = float(testing_cfg.get("frame_win_s", 1.0))
    win, hop = int(win_s * rate), int(float(testing_cfg.get("frame_hop_s", win_s)) * rate)
    sdrs = None
    for j, n_tracks, refs, separations in _musdbhq_tracks(model, testing_cfg, device):
        if sdrs is None:
            sdrs = np.zeros((refs.shape[0], n_tracks))
        sdrs[:, j] = calc_frame_sdr(refs, separations, win, hop)[0].tolist()          # the track's one read-back
        _print_track(model, j, n_tracks, sdrs[:, j])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)              # a source without a valid window in any track: NaN, as museval
        sdrs = np.nanmedian(sdrs, axis=1)
    return (float(np.mean(sdrs)),) + tuple(float(v) for v in sdrs)


def val(argv=None):
    import sys
    if argv is not None:
        sys.argv[1:] = argv
    args = argument_handler()
    if args.use_cpu or not torch.cuda.is_available():
        raise RuntimeError("fqss_amd evaluates on ROCm devices only (no CPU fallback; oracle/ is the CPU checker)")
    conf = yaml.safe_load(open(args.yml_path))
    model_cfg = conf["model_cfg"]
    model = create_pretrained_model(model_cfg)
    enable_observer(model, False)
    model.to("cuda").eval()
    assert not (not model_cfg["quantization"].get("qat", False) and (model.n_splitter > 1 or model.n_splitter > 1)), \
        "No support for splitter/combiner with non QAT model."
    dataset_cfg, testing_cfg = conf["dataset_cfg"], conf.get("testing_cfg", {})
    if dataset_cfg["name"] == "librimix":
        sisnr, imp, sdr, stoi, bss = val_librimix(model, model_cfg, dataset_cfg, testing_cfg, "cuda")
    elif dataset_cfg["name"] == "synthetic":
        bss = None
        sisnr, imp, sdr, stoi = val_synthetic(model, model_cfg, dataset_cfg, testing_cfg, "cuda")
    elif dataset_cfg["name"] == "musdbhq":
        if not testing_cfg.get("NSDR", False):
            if testing_cfg.get("frame_sdr", False):
                res = val_musdbhq_frames(model, testing_cfg, "cuda")
                print(",".join(["SDR={:0.2f}".format(res[0])] + ["SDR_{}={:0.2f}".format(s.upper(), v) for s, v in zip(model.sources, res[1:])]))
                return res
            raise NotImplementedError("dataset musdbhq: val.py:134-178 scores with the third-party `museval` package (absent here); "
                                      "testing_cfg.NSDR: true is served (val_musdbhq_nsdr), and testing_cfg.frame_sdr: true gives "
                                      "museval's SDR restated (val_musdbhq_frames)")
        res = val_musdbhq_nsdr(model, testing_cfg, "cuda")
        # the reference's line, its SNDR_VOCALS spelling included (val.py:221)
        print(",".join(["NSDR={:0.2f}".format(res[0])] + ["{}_{}={:0.2f}".format("SNDR" if s == "vocals" else "NSDR", s.upper(), v)
                                                         for s, v in zip(model.sources, res[1:])]))
        return res
    else:
        assert False, "Dataset {} is not supported!".format(dataset_cfg["name"])
    print("SI-SDR={:0.2f},SI-SDR-imp={:0.2f},SDR={:0.2f},STOI={:0.3f}".format(sisnr, imp, sdr, stoi)
          + (",SIR={:0.2f},SAR={:0.2f}".format(*bss) if bss is not None else ""))
    return sisnr, imp


if __name__ == "__main__":
    val()
