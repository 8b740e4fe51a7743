"""WAV stem folders for the htdemucs env, with demucs' augmentation chain on the device.

The reference's shipped configs/htdemucs.yaml trains from folders of WAV stems (`dset.musdb` / `dset.wav`) through demucs'
`wav.get_wav_datasets` / `get_musdb_wav_datasets` and augments every batch on the device (solver.py:60-69, 314-318: Shift,
FlipChannels, FlipSign, Scale, Remix).  demucs is third party and absent here, so its behaviour is RESTATED in this module; parity
with demucs itself is not pinned by any test.  What is kept:

  layout    `dset.wav: <root>`                     <root>/train/<track>/<source>.wav and <root>/valid/<track>/<source>.wav
            `dset.musdb: <root>`, `use_musdb`      tracks under <root>/train; the validation tracks are named by `dset.valid_tracks`
                                                   (demucs takes that list from the third-party `musdb` package)
  reading   the standard `wave` module: 16-bit PCM at `dset.samplerate` with `dset.channels` channels, every stem of a track of one
            length; anything else raises and names the file (no resampling, no channel conversion).  Samples stay int16 from the
            file to the device: the int16 block of a batch is a view of the prefetcher's pinned buffer.
  examples  training: seg = int(samplerate * segment), stride = int(samplerate * shift); a track of L samples gives 1 example when
            L < seg, else ceil((L - seg) / stride) + 1; example k is [k * stride, k * stride + seg), zero-padded behind the track.
            The Shift augmentation crops `stride` samples, so a step sees seg - stride samples.  shift 0 / absent: hop seg, no crop.
  normalize per-track mean / std of the mono track (channel mean of mixture.wav when the folder has one, else of the stems' sum; std
            with Bessel's correction, as torch.std in demucs' metadata), accumulated in fp64 over the whole track in blocks, cached in
            a JSON file keyed by path, size and mtime.
  augment   `draw_augment` folds the chain into one table row per output (item, source): source item, offset, channel swap, signed
            gain.  One fused kernel (kernels.hd_augment_mix) decodes, normalises, applies the row and sums the stems.

Validation departs from the reference ON PURPOSE: the reference validates whole tracks through demucs' `apply_model` (split /
overlap-add inference) against `mixture.wav`; here the validation set is consecutive windows of the training length over each
validation track, un-augmented (identity table), the mixture being the left-to-right sum of the stems.

`augment.repitch.proba > 0` is refused: it needs the external `soundstretch` program."""
import json
import math
import os
import wave
from typing import NamedTuple

import numpy as np
import torch

from ... import kernels as K

MIXTURE = "mixture"
CACHE_NAME = "wav_metadata.json"
_STAT_BLOCK = 1 << 20           # frames per block of the mean / std pass


class AugmentTable(NamedTuple):
    """one row per output (b, s): sources[b, s] = gain * stem s of item src_b, shifted by off, channels swapped when flip"""
    src_b: torch.Tensor         # [B, S] int64
    off: torch.Tensor           # [B, S] int64
    flip: torch.Tensor          # [B, S] int64, 0 | 1
    gain: torch.Tensor          # [B, S] float32, the sign included


class SeededBatch(list):
    """an index list that carries the seed of its position in the run (`batch_seed`): the batch is a pure function of it"""

    def __init__(self, indices, seed):
        super().__init__(indices)
        self.seed = int(seed)


def batch_seed(seed, epoch, idx, rank=0, world=1):
    """the generator seed of batch `idx` of `epoch` on `rank` (the form Solver._batch uses for the synthetic stems)"""
    return int(seed) * 1000003 + (int(epoch) * (1 << 20) + int(idx)) * int(world) + int(rank)


def identity_table(B, S):
    z = torch.zeros(B, S, dtype=torch.int64)
    return AugmentTable(torch.arange(B, dtype=torch.int64)[:, None].expand(B, S).contiguous(), z, z.clone(), torch.ones(B, S, dtype=torch.float32))


def check_augment_cfg(cfg, batch_size=None):
    """refusals that do not depend on a draw: repitch, and a batch the remix groups do not divide"""
    cfg = cfg or {}
    if float((cfg.get("repitch") or {}).get("proba") or 0) > 0:
        raise NotImplementedError("augment.repitch.proba > 0: repitch needs the external `soundstretch` program and is not built "
                                  "(set augment.repitch.proba: 0)")
    remix = cfg.get("remix") or {}
    if batch_size is not None and float(remix.get("proba") or 0) > 0:
        g = int(remix.get("group_size") or batch_size)
        if g < 1 or batch_size % g != 0:
            raise ValueError(f"augment.remix.group_size {g} does not divide the per-GPU batch {batch_size}")


def draw_augment(B, S, C, shift, cfg, generator):
    """The table of one training batch: demucs' chain Shift -> FlipChannels -> FlipSign -> Scale -> Remix (augment.py of demucs,
    restated; solver.py:60-69 builds it from the `augment` block), every draw from `generator`, in this order:
      shift   off = randint(0, shift) per (b, s), one per item when `shift_same`; shift == 0: no draw, off = 0
      flip    (`flip`) C == 2: a swap bit per (b, s); then a sign per (b, s)
      scale   one uniform draw against `scale.proba`, then (when it hits) uniform(min, max) per (b, s)
      remix   one uniform draw against `remix.proba`, then (when it hits) per group of `group_size` consecutive items and per source
              an independent permutation of the group's items (argsort of uniform draws)
    Remix moves whole augmented (item, source) rows, so the row of output (b, s) is the row drawn for (src_b[b, s], s).
    gain = sign * scale: the sign is exact, one rounding is left for the kernel's multiply."""
    cfg = cfg or {}
    check_augment_cfg(cfg)
    g = generator
    shift = int(shift)
    if shift > 0:
        off = torch.randint(0, shift, (B, 1) if cfg.get("shift_same") else (B, S), generator=g).expand(B, S).contiguous()
    else:
        off = torch.zeros(B, S, dtype=torch.int64)
    flip = torch.zeros(B, S, dtype=torch.int64)
    gain = torch.ones(B, S, dtype=torch.float32)
    if cfg.get("flip"):
        if C == 2:
            flip = torch.randint(0, 2, (B, S), generator=g)
        gain = (2 * torch.randint(0, 2, (B, S), generator=g) - 1).to(torch.float32)
    scale = cfg.get("scale") or {}
    if float(torch.rand((), generator=g)) < float(scale.get("proba") or 0):
        lo, hi = float(scale.get("min", 0.25)), float(scale.get("max", 1.25))
        gain = gain * (lo + (hi - lo) * torch.rand(B, S, generator=g, dtype=torch.float64)).to(torch.float32).clamp_(lo, hi)
    src_b = torch.arange(B, dtype=torch.int64)[:, None].expand(B, S).contiguous()
    remix = cfg.get("remix") or {}
    if float(torch.rand((), generator=g)) < float(remix.get("proba") or 0):
        gs = int(remix.get("group_size") or B)
        if gs < 1 or B % gs != 0:
            raise ValueError(f"augment.remix: batch size {B} is not divisible by group size {gs}")
        perm = torch.argsort(torch.rand(B // gs, gs, S, generator=g), dim=1)                    # [groups, gs, S], within the group
        src_b = (perm + gs * torch.arange(B // gs, dtype=torch.int64)[:, None, None]).reshape(B, S)
        off, flip, gain = off.gather(0, src_b), flip.gather(0, src_b), gain.gather(0, src_b)
    return AugmentTable(src_b, off, flip, gain)


# ---- files ------------------------------------------------------------------------------------------------------------------------
def _open_checked(path, samplerate, channels):
    """an open wave reader of a file in the one format that is read; the caller closes it"""
    try:
        w = wave.open(path, "rb")
    except FileNotFoundError:
        raise FileNotFoundError(f"{path}: missing stem") from None
    except (wave.Error, EOFError) as e:
        raise ValueError(f"{path}: not a PCM WAV file the `wave` module reads ({e})") from None
    bad = None
    if w.getcomptype() != "NONE" or w.getsampwidth() != 2:
        bad = f"{8 * w.getsampwidth()}-bit {w.getcomptype()} samples (16-bit PCM is read)"
    elif w.getframerate() != samplerate:
        bad = f"sample rate {w.getframerate()}, dset.samplerate is {samplerate} (no resampling)"
    elif w.getnchannels() != channels:
        bad = f"{w.getnchannels()} channels, dset.channels is {channels} (no channel conversion)"
    if bad:
        w.close()
        raise ValueError(f"{path}: {bad}")
    return w


def _signature(track_dir, sources):
    """(file name, size, mtime) of every file the metadata of a track depends on -- os.stat only, no file is opened"""
    sig = []
    for name in list(sources) + [MIXTURE]:
        p = os.path.join(track_dir, name + ".wav")
        try:
            st = os.stat(p)
        except FileNotFoundError:
            if name == MIXTURE:
                continue
            raise FileNotFoundError(f"{p}: missing stem") from None
        sig.append([name, int(st.st_size), int(st.st_mtime_ns)])
    return sig


def _track_metadata(track_dir, sources, samplerate, channels, want_stats):
    """length in frames (every stem checked: format and equal lengths) and, when asked for, mean / std of the mono track in fp64:
    one pass in blocks, block moments merged by Chan's update"""
    files = [os.path.join(track_dir, s + ".wav") for s in sources]
    readers = []
    try:
        for p in files:
            readers.append(_open_checked(p, samplerate, channels))
        L = readers[0].getnframes()
        for p, w in zip(files, readers):
            if w.getnframes() != L:
                raise ValueError(f"{p}: {w.getnframes()} frames, {files[0]} has {L} (the stems of a track have one length)")
        if L == 0:
            raise ValueError(f"{files[0]}: empty track")
        if not want_stats:
            return L, None, None
        mixture = os.path.join(track_dir, MIXTURE + ".wav")
        if os.path.exists(mixture):
            for w in readers:
                w.close()
            readers = [_open_checked(mixture, samplerate, channels)]
            if readers[0].getnframes() != L:
                raise ValueError(f"{mixture}: {readers[0].getnframes()} frames, the stems have {L}")
        n, mean, m2 = 0, 0.0, 0.0
        for pos in range(0, L, _STAT_BLOCK):
            k = min(_STAT_BLOCK, L - pos)
            tot = np.zeros((k, channels), dtype=np.int64)
            for w in readers:
                tot += np.frombuffer(w.readframes(k), dtype="<i2").reshape(k, channels)
            mono = tot.sum(axis=1).astype(np.float64) / (channels * 32768.0)
            bm = float(mono.mean())
            bm2 = float(((mono - bm) ** 2).sum())
            delta = bm - mean
            mean += delta * k / (n + k)
            m2 += bm2 + delta * delta * n * k / (n + k)
            n += k
        std = math.sqrt(m2 / (n - 1)) if n > 1 else 0.0
        if not std > 0.0:
            raise ValueError(f"{track_dir}: the track's standard deviation is {std} (dset.normalize divides by it)")
        return L, mean, std
    finally:
        for w in readers:
            w.close()


def load_metadata(track_dirs, sources, samplerate, channels, normalize, cache_file):
    """{track_dir: (length, mean, std)}; entries of `cache_file` whose files are unchanged (path, size, mtime) are reused without
    opening a stem, the rest are read and the file is rewritten"""
    cache = {}
    if cache_file and os.path.exists(cache_file):
        try:
            with open(cache_file) as f:
                cache = json.load(f)
        except (OSError, ValueError):
            cache = {}
    out, dirty = {}, False
    for d in track_dirs:
        key = os.path.abspath(d)
        sig = _signature(d, sources)
        ent = cache.get(key)
        if not (isinstance(ent, dict) and ent.get("files") == sig and ent.get("samplerate") == samplerate and ent.get("channels") == channels
                and (not normalize or ent.get("std") is not None)):
            L, mean, std = _track_metadata(d, sources, samplerate, channels, normalize)
            ent = cache[key] = {"files": sig, "samplerate": samplerate, "channels": channels, "length": L, "mean": mean, "std": std}
            dirty = True
        if normalize and not float(ent["std"]) > 0.0:
            raise ValueError(f"{d}: the track's standard deviation is {ent['std']} (dset.normalize divides by it)")
        out[d] = (int(ent["length"]), ent["mean"], ent["std"])
    if dirty and cache_file:
        os.makedirs(os.path.dirname(os.path.abspath(cache_file)), exist_ok=True)
        tmp = f"{cache_file}.{os.getpid()}.tmp"
        with open(tmp, "w") as f:
            json.dump(cache, f)
        os.replace(tmp, cache_file)
    return out


def _list_tracks(root):
    if not os.path.isdir(root):
        raise FileNotFoundError(f"{root}: no such track folder")
    return sorted(n for n in os.listdir(root) if os.path.isdir(os.path.join(root, n)))


def configured(dset):
    """does the `dset` block name a WAV dataset?  (`name: synthetic` keeps the seeded synthetic stems)"""
    return dset.get("name") != "synthetic" and bool(dset.get("wav") or (dset.get("use_musdb") and dset.get("musdb")))


def split_tracks(dset):
    """(training track folders, validation track folders) of the `dset` block"""
    if dset.get("wav2"):
        raise NotImplementedError("dset.wav2 (a second custom dataset) is not built")
    if dset.get("wav") and dset.get("use_musdb") and dset.get("musdb"):
        raise NotImplementedError("dset.wav together with dset.use_musdb: one dataset is read; set use_musdb: false or clear dset.wav")
    if dset.get("wav"):
        root = dset["wav"]
        return tuple([os.path.join(root, part, n) for n in _list_tracks(os.path.join(root, part))] for part in ("train", "valid"))
    root = os.path.join(dset["musdb"], "train")
    valid = dset.get("valid_tracks")
    if not valid:
        raise ValueError("dset.valid_tracks is required with dset.use_musdb: the names of the validation tracks under <musdb>/train "
                         "(demucs takes them from the third-party `musdb` package)")
    names = _list_tracks(root)
    missing = [n for n in valid if n not in names]
    if missing:
        raise FileNotFoundError(f"{root}: dset.valid_tracks names no folder for {missing}")
    return [os.path.join(root, n) for n in names if n not in valid], [os.path.join(root, n) for n in valid]


class WavStems:
    """the windows of a list of track folders.  `train`: overlapping examples of `seg` samples, augmented by the table drawn from the
    batch's seed and cropped to seg - stride; otherwise consecutive windows of seg - stride samples, identity table."""

    def __init__(self, track_dirs, sources, samplerate, channels, segment, shift=0, normalize=False, cache_file=None, train=True,
                 augment=None, max_examples=None, device="cuda"):
        self.tracks, self.sources, self.samplerate, self.channels = list(track_dirs), list(sources), int(samplerate), int(channels)
        self.normalize, self.train, self.augment, self.device = bool(normalize), bool(train), augment or {}, device
        if not 1 <= len(self.sources) <= 8:
            raise ValueError(f"dset.sources: {len(self.sources)} sources (1 to 8 are built)")
        if self.channels not in (1, 2):
            raise ValueError(f"dset.channels: {self.channels} (1 | 2)")
        if not self.tracks:
            raise ValueError("no track folder to read")
        check_augment_cfg(self.augment)
        seg = int(self.samplerate * segment)
        self.stride = int(self.samplerate * (shift or 0))
        if seg <= self.stride or seg < 1:
            raise ValueError(f"dset.segment ({seg} samples) must be longer than dset.shift ({self.stride} samples)")
        self.T_out = seg - self.stride                       # what a step sees
        self.T_in = seg if self.train else self.T_out        # what an example holds
        self.hop = (self.stride or seg) if self.train else self.T_out
        meta = load_metadata(self.tracks, self.sources, self.samplerate, self.channels, self.normalize, cache_file)
        self.length = [meta[d][0] for d in self.tracks]
        self.mean = [meta[d][1] for d in self.tracks]
        self.std = [meta[d][2] for d in self.tracks]
        counts = [1 if L < self.T_in else -(-(L - self.T_in) // self.hop) + 1 for L in self.length]
        self._first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self._n = int(self._first[-1]) if max_examples is None else min(int(self._first[-1]), int(max_examples))

    def __len__(self):
        return self._n

    # ---- host side: which files, which window, the int16 block, the table -------------------------------------------------
    def example(self, i):
        """(track index, first sample) of example i"""
        if not 0 <= i < self._n:
            raise IndexError(i)
        k = int(np.searchsorted(self._first, i, side="right")) - 1
        return k, (i - int(self._first[k])) * self.hop

    def stage_elems(self, batch_size):
        """float32 elements of the pinned staging buffer a batch needs: its int16 block is a view of that buffer"""
        return (batch_size * len(self.sources) * self.T_in * self.channels + 1) // 2

    def host_batch(self, indices, stage=None):
        """(pcm int16 [B, S, T_in, C] -- a view of `stage` when one is given --, table, mean [B] | None, std [B] | None), all on the
        host: the files' samples as they are, zeros behind the end of a track"""
        B, S, C, T = len(indices), len(self.sources), self.channels, self.T_in
        n = B * S * T * C
        if stage is not None:
            if stage.numel() < self.stage_elems(B):
                raise ValueError(f"staging buffer of {stage.numel()} elements, {self.stage_elems(B)} needed")
            pcm = stage.view(torch.int16)[:n].view(B, S, T, C)
        else:
            pcm = torch.empty(B, S, T, C, dtype=torch.int16)
        hv = pcm.numpy()
        where = [self.example(int(i)) for i in indices]
        for b, (k, start) in enumerate(where):
            got = max(0, min(T, self.length[k] - start))
            for s, name in enumerate(self.sources):
                path = os.path.join(self.tracks[k], name + ".wav")
                w = _open_checked(path, self.samplerate, C)
                try:
                    if w.getnframes() != self.length[k]:
                        raise ValueError(f"{path}: {w.getnframes()} frames, {self.length[k]} when the track was indexed")
                    w.setpos(start)
                    hv[b, s, :got] = np.frombuffer(w.readframes(got), dtype="<i2").reshape(got, C)
                finally:
                    w.close()
                hv[b, s, got:] = 0
        if self.train:
            seed = getattr(indices, "seed", None)
            if seed is None:
                raise ValueError("a training batch carries the seed of its position (SeededBatch(indices, batch_seed(...)))")
            table = draw_augment(B, S, C, self.stride, self.augment, torch.Generator().manual_seed(seed))
        else:
            table = identity_table(B, S)
        mean = std = None
        if self.normalize:
            mean = torch.tensor([self.mean[k] for k, _ in where], dtype=torch.float64).to(torch.float32)
            std = torch.tensor([self.std[k] for k, _ in where], dtype=torch.float64).to(torch.float32)
        return pcm, table, mean, std

    # ---- device side ----------------------------------------------------------------------------------------------------------
    def batch(self, indices, stage=None):
        """(mix [B, C, T_out], sources [B, S, C, T_out]) on the device, enqueued on the calling thread's current stream: one upload of
        the int16 block (asynchronous through the caller's pinned `stage`), one fused launch"""
        pcm, table, mean, std = self.host_batch(indices, stage)
        dev = pcm.to(self.device, non_blocking=stage is not None)
        return K.hd_augment_mix(dev, self.T_out, table.src_b, table.off, table.flip, table.gain, mean, std)


def build_datasets(conf, device="cuda"):
    """(training set, validation set) of a configuration whose `dset` block names a WAV dataset"""
    d = conf["dset"]
    train_dirs, valid_dirs = split_tracks(d)
    cache = os.path.join(conf["work_dir"], CACHE_NAME)
    kw = dict(sources=d["sources"], samplerate=d["samplerate"], channels=d["channels"], segment=d["segment"], shift=d.get("shift") or 0,
              normalize=bool(d.get("normalize")), cache_file=cache, device=device)
    train = WavStems(train_dirs, train=True, augment=conf.get("augment"), **kw)
    valid = WavStems(valid_dirs, train=False, max_examples=d.get("valid_samples"), **kw)
    return train, valid
