"""The fused stem kernel of the htdemucs env (kernels.hd_augment_mix) against the same result built from stock torch device ops, fed
the same uploaded int16 block, at the reference's per-GPU shape (batch 4, 4 stereo sources, 10 s windows cropped to 9 s at 44.1 kHz).
One device, one run: device events, warmed up, median of 20 alternating repeats; prints one JSON line with both times (`kernel_only_ms`, the
launch alone, is the device figure that `torch_chain_ms` is compared with; `wrapper_ms` spans the wrapper as the loader calls it, host
range checks and pageable table upload included, so it is host latency rather than device work) and the kernel's achieved bytes per second (the bytes the algorithm needs: the int16 frames it reads once, the stems and the mixture it writes).
    python tools/hd_loader_probe.py [B] [S] [seconds_in] [seconds_out]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fqss_amd import _lib, kernels as K  # noqa: E402
from fqss_amd.train_env.htdemucs_musdbhq.wav_dataset import draw_augment  # noqa: E402

SR, C, REPEATS, WARMUP = 44100, 2, 20, 3


def torch_chain(pcm, T_out, src_b, off, flip, gain, mean, std):
    """the statement of include/fqss.h with stock ops; the index tensors are on the device already"""
    B, S, T_in, _ = pcm.shape
    x = pcm.to(torch.float32) * 2.0 ** -15
    x = (x - mean.view(B, 1, 1, 1)) / std.view(B, 1, 1, 1)
    t = off[..., None] + torch.arange(T_out, device=pcm.device)
    x = x[src_b[..., None], torch.arange(S, device=pcm.device)[None, :, None], t]              # [B, S, T_out, C]
    ch = torch.arange(C, device=pcm.device)[None, None, None, :] ^ flip[..., None, None]
    x = torch.gather(x, 3, ch.expand(B, S, T_out, C))
    x = x * gain[..., None, None]
    sources = x.permute(0, 1, 3, 2).contiguous()
    return sources.sum(dim=1), sources


def main(argv):
    assert torch.cuda.is_available(), "the probe measures on a ROCm device"
    B, S = (int(argv[0]) if argv else 4), (int(argv[1]) if len(argv) > 1 else 4)
    T_in = int(SR * (float(argv[2]) if len(argv) > 2 else 10.0))
    T_out = int(SR * (float(argv[3]) if len(argv) > 3 else 9.0))
    g = torch.Generator().manual_seed(0)
    pcm = torch.randint(-32768, 32768, (B, S, T_in, C), generator=g, dtype=torch.int32).to(torch.int16).pin_memory().cuda(non_blocking=True)
    cfg = {"flip": True, "scale": {"proba": 1, "min": 0.25, "max": 1.25}, "remix": {"proba": 1, "group_size": B}}
    table = draw_augment(B, S, C, T_in - T_out + 1, cfg, g)
    mean, std = (torch.rand(B, generator=g) - 0.5) * 0.01, 0.1 + torch.rand(B, generator=g) * 0.2
    dev = [t.cuda() for t in (*table, mean, std)]
    sources = torch.empty(B, S, C, T_out, device="cuda")
    mix = torch.empty(B, C, T_out, device="cuda")

    def fused():
        return K.hd_augment_mix(pcm, T_out, *table, mean, std, sources=sources, mix=mix)

    di = [t.to(torch.int32).cuda() for t in table[:3]]

    def kernel_only():          # the launch alone: the table is on the device already (the wrapper's host checks and upload left out)
        _lib.call("fqss_hd_augment_mix", pcm.data_ptr(), dev[4].data_ptr(), dev[5].data_ptr(), di[0].data_ptr(), di[1].data_ptr(), di[2].data_ptr(),
                  dev[3].data_ptr(), sources.data_ptr(), mix.data_ptr(), B, S, C, T_in, T_out, 1, torch.cuda.current_stream().cuda_stream)

    def chain():
        return torch_chain(pcm, T_out, *dev)

    m1, s1 = fused()
    m2, s2 = chain()
    torch.cuda.synchronize()
    same_sources, mix_err = bool(torch.equal(s1, s2)), float((m1 - m2).abs().max())
    times = {"fused": [], "kernel": [], "torch": []}
    for i in range(WARMUP + REPEATS):
        for name, fn in (("fused", fused), ("kernel", kernel_only), ("torch", chain)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= WARMUP:
                times[name].append(a.elapsed_time(b))
    t_f, t_k, t_t = (statistics.median(times[k]) for k in ("fused", "kernel", "torch"))
    nbytes = B * S * T_out * C * 2 + (B * S * C * T_out + B * C * T_out) * 4
    print(json.dumps({"shape": {"B": B, "S": S, "C": C, "T_in": T_in, "T_out": T_out}, "kernel_only_ms": round(t_k, 4), "wrapper_ms": round(t_f, 4),
                      "torch_chain_ms": round(t_t, 4), "torch_chain_over_kernel_only": round(t_t / t_k, 2), "kernel_bytes": nbytes, "kernel_GBps": round(nbytes / t_k / 1e6, 1),
                      "kernel_only_ms_min_max": [round(min(times["kernel"]), 4), round(max(times["kernel"]), 4)],
                      "torch_ms_min_max": [round(min(times["torch"]), 4), round(max(times["torch"]), 4)],
                      "sources_equal_torch_chain": same_sources, "mix_max_abs_diff_vs_torch_sum": mix_err}))


if __name__ == "__main__":
    main(sys.argv[1:])
