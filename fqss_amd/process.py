"""8-bit input splitter / output combiner on MI355X (reference: process.py:10-52).

`preprocess` = global max-normalise + MSB/LSB floor-quantised channels (HIP: fqss_minmax + fqss_splitter2),
`postprocess` = `x0 + x1 * 2^-8` (HIP: fqss_axpby).  The evaluation helpers of the reference's process.py run on the device too:
chunked overlap-add inference with per-chunk source re-ordering, SI-SNR (fqss_sisnr_matrix), SDR (fqss_sdr) and STOI (fqss_stoi) of
`metric_evaluation`.  STOI is opt-in (`with_stoi=True`; pystoi is third party and absent: restated, NaN by default).
"""
import torch

from . import _lib
from . import kernels as K
from . import ops


def quantize(x, threshold=1.0, n_bits=8, sign=True):
    """floor quantizer of the splitter (process.py:10-14); served by the splitter kernel only"""
    raise NotImplementedError("process.quantize is fused inside fqss_splitter2; call preprocess(n_splitter=2)")


def preprocess(x, n_splitter=1, n_bits=8, sign=True, normalize=True):
    if x.dim() == 2:
        x = x.unsqueeze(1)
    if n_splitter <= 1:
        return x
    if n_splitter != 2 or n_bits != 8 or not sign:
        raise NotImplementedError("the splitter kernel serves n_splitter=2, 8 bit, signed")
    if normalize and x.shape[1] == 1 and x.dim() == 3:
        return ops.splitter2_rows(x) if ops.SPLIT_PER_ITEM else ops.splitter2(x)
    if ops.SPLIT_PER_ITEM:
        raise NotImplementedError("ops.split_per_item serves [B, 1, T] waveforms (fqss_splitter2_rows); the multi-channel / "
                                  "normalize=False splitter of HTDemucs has one threshold for the whole tensor")
    # multi-channel / multi-dimensional inputs (HTDemucs: [B, A, Fr, T] spectrogram, [B, A, T] waveform): the flattened
    # [B, 2, A*...] result is torch.cat([msb, lsb], dim=1)
    with torch.no_grad():
        y = K.splitter2(x, normalize=normalize)
    return y.view(x.shape[0], 2 * x.shape[1], *x.shape[2:])


def postprocess(x, n_combiner=1, n_bits=8, sign=True):
    """x: [n_combiner, batch, sources, audio_channels, T]"""
    if n_combiner == 1:
        y = x.squeeze(0)
    elif n_combiner == 2 and n_bits == 8 and sign:
        y = ops.Combine2.apply(x[0], x[1])
    else:
        raise NotImplementedError("the combiner kernel serves n_combiner in {1,2}, 8 bit, signed")
    if y.dim() <= 4 and y.shape[-2] == 1:
        y = y.squeeze(-2)
    return y


# ---------------------------------------------------------------------------------------------------------------------------
# evaluation side: process.py:105-194 of the reference on the device
# ---------------------------------------------------------------------------------------------------------------------------
def si_snr(est, ref):
    """SI-SNR in dB between matching rows of est / ref [S, L] (torchmetrics' ScaleInvariantSignalNoiseRatio, third party:
    zero-mean SI-SDR with eps = 2^-23, restated; process.py:119, 137)"""
    return torch.diagonal(K.sisnr_matrix(est.reshape(-1, est.shape[-1]), ref.reshape(-1, ref.shape[-1])))


def swap_channel_order(sep_tensor, clean_tensor):
    """process.swap_channel_order (process.py:105-125): every estimate goes to the target it matches best (sign flipped when it
    moves); the decision is taken on the device (fqss_sisnr_matrix), the copy is the weighted overlap-add's with weight 1"""
    n_src = clean_tensor.shape[0]
    if n_src == 1:
        return sep_tensor
    L = sep_tensor.shape[-1]
    sep2 = sep_tensor.reshape(n_src, -1).contiguous()
    _, mp = K.sisnr_matrix(sep2, clean_tensor.reshape(n_src, -1), want_map=True)
    idx = mp[:, 0].long()
    out = sep2[idx] * mp[:, 1:2].to(sep2.dtype)        # (a gather of S rows and a sign: no arithmetic on the samples)
    return out.reshape(sep_tensor.shape)


def _model_infer_batched(model, mix, num_srcs, segment, overlap, target, chunk_batch):
    """the chunks of one utterance through the model `chunk_batch` at a time: what the chunk-by-chunk loop of `model_infer` computes
    (per-chunk splitter threshold, per-chunk re-ordering, the same overlap-add in the same order) in ceil(N / G) forwards instead of N;
    nothing is read back to the host"""
    G = int(chunk_batch)
    if G < 1:
        raise ValueError(f"chunk_batch must be a positive number of chunks, got {chunk_batch!r}")
    channels, length = mix.shape
    if channels > 1:
        raise NotImplementedError("chunk_batch serves one-channel mixtures (the waveform models); multi-channel chunked inference "
                                  "runs chunk by chunk (chunk_batch=None)")
    segment = int(segment)
    stride = int((1 - overlap) * segment)
    if not 1 <= stride <= segment:
        raise ValueError(f"chunk_batch needs 1 <= int((1 - overlap) * segment) <= segment, got a hop of {stride}")
    mix = mix.contiguous()
    n_chunks = len(range(0, length, stride))
    n_pad = -(-n_chunks // G) * G
    want_map = target is not None and num_srcs > 1
    maps = torch.empty(n_pad, num_srcs, 2, device=mix.device, dtype=torch.int32) if want_map else None
    db = torch.empty(G, num_srcs, num_srcs, device=mix.device, dtype=torch.float32) if want_map else None
    buf = None
    for k0 in range(0, n_chunks, G):
        chunks = K.chunk_gather(mix, segment, stride, k0, G)
        with torch.no_grad(), ops.split_per_item(True):
            y = model(chunks).detach()
        y = y.reshape(G, num_srcs, y.shape[-1])
        n = min(y.shape[-1], segment)
        if buf is None:     # a model that returns fewer than `segment` samples is zero-padded, as the whole-utterance call pads it
            buf = (torch.zeros if n < segment else torch.empty)(n_pad, num_srcs, segment, device=mix.device, dtype=torch.float32)
        buf[k0:k0 + G, :, :n].copy_(y[..., :n])
        if want_map:
            K.sisnr_chunks(buf[k0:k0 + G], target.reshape(num_srcs, -1), stride, k0, db=db, mp=maps[k0:k0 + G])
    return K.infer_ola_chunks(buf, maps, length, stride)


def model_infer(model, mix, n_srcs=1, segment=None, overlap=0.25, device="cuda", target=None, chunk_batch=None):
    """process.model_infer (process.py:156-194): whole-utterance inference, or chunks of `segment` samples hopped by
    (1 - overlap) * segment, re-ordered per chunk against `target` and blended with the triangular window.  mix [channels, length];
    returns [n_srcs, (channels,) length] on the device (the reference returns a CPU tensor).  chunk_batch=G (opt-in) sends the chunks
    through the model G at a time (`_model_infer_batched`); None runs them one by one."""
    if str(device) == "cpu" and _lib.BACKEND != "cpu":
        raise RuntimeError("fqss_amd runs on ROCm devices only (oracle/ is the CPU checker)")
    mix = mix.to(device)
    if segment and chunk_batch is not None:
        num_srcs = model.n_srcs if hasattr(model, "n_srcs") else n_srcs
        return _model_infer_batched(model, mix, num_srcs, segment, overlap, None if target is None else target.to(device), chunk_batch)
    if not segment:
        with torch.no_grad():
            out = model(mix.unsqueeze(0)).detach()[0]
        pad = mix.size(-1) - out.size(-1)
        return torch.nn.functional.pad(out, (0, pad)) if pad > 0 else out
    channels, length = mix.shape
    num_srcs = model.n_srcs if hasattr(model, "n_srcs") else n_srcs
    out = torch.zeros((num_srcs, channels, length) if channels > 1 else (num_srcs, length), device=mix.device)
    sum_weight = torch.zeros(length, device=mix.device)
    stride = int((1 - overlap) * segment)
    if target is not None:
        target = target.to(device)
    for start in range(0, length, stride):
        stop = min(start + segment, length)
        n = stop - start
        chunk = mix[..., start:stop]
        if n < segment:
            padded = torch.zeros(channels, segment, device=mix.device)
            padded[:, :n].copy_(chunk)
            chunk = padded
        chunk_out = model_infer(model, chunk, device=device)[..., :n].contiguous()
        mp = None
        if target is not None and num_srcs > 1:
            _, mp = K.sisnr_matrix(chunk_out.reshape(num_srcs, -1), target[..., start:start + n].reshape(num_srcs, -1), want_map=True)
        K.infer_ola(chunk_out, mp, out, sum_weight, start, n, segment)
    K.infer_normalize(out, sum_weight)
    return out


def sdr(est, ref, filter_length=512, zero_mean=False, load_diag=None):
    """SDR in dB between matching rows of est / ref [..., L] (torchmetrics' SignalDistortionRatio with its defaults, third party: the
    fast_bss_eval definition restated -- both signals normalised, `filter_length` lags of auto- and cross-correlation, a Toeplitz solve;
    process.py:145).  Leading dimensions are flattened to pairs; returns fp64 [pairs] on the device, NaN where the target is silent."""
    return K.sdr(est.reshape(-1, est.shape[-1]), ref.reshape(-1, ref.shape[-1]), filter_length=filter_length, zero_mean=zero_mean,
                 load_diag=load_diag)


def stoi(est, ref, sample_rate):
    """Short-time objective intelligibility between matching rows of est / ref [..., L] sampled at `sample_rate` (torchmetrics'
    ShortTimeObjectiveIntelligibility(fs)(preds=est, target=ref) = pystoi.stoi(ref, est, fs), third party: the published definition
    restated, see fqss_stoi in include/fqss.h; process.py:147).  Leading dimensions are flattened to pairs; returns fp64 [pairs] on the
    device.  Rates served: 8000, 10000, 16000 Hz."""
    return K.stoi(est.reshape(-1, est.shape[-1]), ref.reshape(-1, ref.shape[-1]), sample_rate)


def metric_evaluation(sep_waveform, clean_waveforms, sample_rate=16000, with_sdr=True, with_stoi=False):
    """(SI-SNR, SDR, STOI) averaged over the sources (process.py:127-154): every estimate is paired with the target of its best SI-SNR
    (first maximum) and the metrics are taken on that pair.  The pairing stays on the device (first-maximum index + gather) and all
    pairs go through one fqss_sdr launch.  A silent matched target makes that pair's SDR, and so the mean, NaN, as numpy.mean does in
    the reference.  with_sdr=False leaves the SDR slot NaN (val.py's mixture baseline uses the SI-SNR slot only).  with_stoi=True fills
    the STOI slot with the mean fqss_stoi of the same pairs at `sample_rate` (one more launch sequence, the same single read-back);
    by default it stays NaN, as it was while pystoi -- third party and absent -- had no restatement here."""
    S = clean_waveforms.shape[0]
    est, clean = sep_waveform.reshape(S, -1), clean_waveforms.reshape(S, -1)
    db = K.sisnr_matrix(est, clean)
    best = db.max(dim=1, keepdim=True).values
    if not with_sdr and not with_stoi:
        return best.mean().item(), float("nan"), float("nan")
    cols = torch.arange(S, device=db.device).expand(S, S)
    first = torch.where(db == best, cols, S).min(dim=1).values          # the first maximum, as the reference's strict `>` scan
    first = torch.where(first < S, first, 0)                            # (a row of NaN: the scan keeps index 0)
    matched = clean[first]
    means = [best.mean().double()]
    if with_sdr:
        means.append(K.sdr(est, matched).mean())
    if with_stoi:
        means.append(K.stoi(est, matched, sample_rate).mean())
    means = torch.stack(means).tolist()                                 # the one read-back
    return means[0], means[1] if with_sdr else float("nan"), means[-1] if with_stoi else float("nan")


# ---------------------------------------------------------------------------------------------------------------------------
# data side: the SNR augmentation of the LibriMix dataset on the device, batched
# ---------------------------------------------------------------------------------------------------------------------------
def generate_2mix_snr(signal1, signal2, snr, clip=True):
    """process.generate_2mix_snr (process.py:77-91) for one pair [T] or a batch [B, T]; snr: a number or a [B] tensor (dB)"""
    one = signal1.dim() == 1
    a, b = signal1.reshape(-1, signal1.shape[-1]), signal2.reshape(-1, signal2.shape[-1])
    s = snr if torch.is_tensor(snr) else torch.full((a.shape[0],), float(snr), device=a.device)
    out = K.snr_mix(a, b, s.to(a.device, torch.float32), 0, clip)
    return out[0] if one else out


def generate_3mix_snr(signal1, signal2, signal3, snr1_23, snr2_3):
    return generate_2mix_snr(signal1, generate_2mix_snr(signal2, signal3, snr2_3), snr1_23)


def generate_mix_noise(sig, noise, snr):
    """process.generate_mix_noise (process.py:98-103)"""
    one = sig.dim() == 1
    a, b = sig.reshape(-1, sig.shape[-1]), noise.reshape(-1, noise.shape[-1])
    s = snr if torch.is_tensor(snr) else torch.full((a.shape[0],), float(snr), device=a.device)
    out = K.snr_mix(a, b, s.to(a.device, torch.float32), 1, True)
    return out[0] if one else out
