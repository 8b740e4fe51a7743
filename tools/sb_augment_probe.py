"""The fused Sepformer-recipe kernel (kernels.sb_augment: roll, re-mix, notch FIR, zeroed chunks, cut) against the same result built
from stock torch device ops (`roll`, `stack` / `sum`, `F.conv1d`, slice assignment, slice) on whole utterances, at the recipe's shape:
a batch of 2 x 10 s at 8 kHz, two sources of different lengths, a 32000-sample window.  One device, one run: device events, warmed up,
median of 20 alternating repeats; prints one JSON line (`kernel_only_ms`: the launch alone with the table on the device already, the
figure `torch_chain_ms` is compared with; `wrapper_ms`: the wrapper as the loader calls it, host checks and the pageable table upload
included, so host latency rather than device work) and the bytes the kernel needs (the window and halo of every source it reads, the
targets and the mixture it writes) per second.
    python tools/sb_augment_probe.py [B] [seconds] [T_out]"""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fqss_amd import _lib, kernels as K  # noqa: E402

SR, REPEATS, WARMUP = 8000, 20, 3


def torch_chain(srcs, shifts, taps, chunks, start, T_out):
    """the statement of include/fqss.h with stock ops on whole utterances; conv1d is a correlation, as the statement is"""
    n = min(s.shape[1] for s in srcs)
    tgt = torch.stack([torch.roll(s, k, dims=1)[:, :n] for s, k in zip(srcs, shifts)], dim=1)
    mix = F.conv1d(tgt.sum(1, keepdim=True), taps.view(1, 1, -1), padding=50)
    for b, row in enumerate(chunks):
        for lo, hi in row:
            mix[b, :, lo:hi] = 0.0
    return mix[..., start:start + T_out].contiguous(), tgt[..., start:start + T_out].contiguous()


def main(argv):
    assert torch.cuda.is_available(), "the probe measures on a ROCm device"
    B = int(argv[0]) if argv else 2
    L = int(SR * (float(argv[1]) if len(argv) > 1 else 10.0))
    T_out = int(argv[2]) if len(argv) > 2 else 32000
    g = torch.Generator().manual_seed(0)
    lengths = [L * 100 // 95, L * 100 // 105]                            # the two sources after speeds 95 and 105
    srcs = [(torch.rand(B, n, generator=g) - 0.5).cuda() for n in lengths]
    n = min(lengths)
    shifts = [int(torch.randint(-8000, 8000, (1,), generator=g)) % m for m in lengths]
    taps = torch.from_numpy(K.notch_taps([0.21, 0.6])).to(torch.float32)
    start = (n - T_out) // 2
    chunks = [[(start + 3000 * c + 500 * b, start + 3000 * c + 500 * b + 1500) for c in range(5)] for b in range(B)]
    taps_d = taps.cuda()
    tab = torch.tensor([len(r) for r in chunks] + [v for r in chunks for lo_hi in r + [(0, 0)] * (K.SB_C_MAX - len(r)) for v in lo_hi],
                       dtype=torch.int32).cuda()
    mix, tgt = torch.empty(B, 1, T_out, device="cuda"), torch.empty(B, 2, T_out, device="cuda")

    def fused():
        return K.sb_augment(srcs, shifts, taps, chunks, start, T_out)

    def kernel_only():          # the launch alone: taps and chunk table on the device already
        _lib.call("fqss_sb_augment", srcs[0].data_ptr(), srcs[1].data_ptr(), None, lengths[0], lengths[1], 0, lengths[0], lengths[1], 0,
                  shifts[0], shifts[1], 0, None, 0, 0, None, 0, 0, taps_d.data_ptr(), tab.data_ptr() + 4 * B, tab.data_ptr(), mix.data_ptr(),
                  tgt.data_ptr(), B, 2, start, T_out, 1, torch.cuda.current_stream().cuda_stream)

    def chain():
        return torch_chain(srcs, shifts, taps_d, chunks, start, T_out)

    m1, t1 = fused()
    m2, t2 = chain()
    kernel_only()
    torch.cuda.synchronize()
    same = bool(torch.equal(t1, t2)) and bool(torch.equal(m1, mix))
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
    nbytes = 4 * B * (2 * (T_out + 100) + 3 * T_out)
    print(json.dumps({"shape": {"B": B, "S": 2, "L": lengths, "T_out": T_out}, "kernel_only_ms": round(t_k, 4), "wrapper_ms": round(t_f, 4),
                      "torch_chain_ms": round(t_t, 4), "torch_chain_over_kernel_only": round(t_t / t_k, 2), "kernel_bytes": nbytes,
                      "kernel_GBps": round(nbytes / t_k / 1e6, 1), "kernel_only_ms_min_max": [round(min(times["kernel"]), 4), round(max(times["kernel"]), 4)],
                      "torch_ms_min_max": [round(min(times["torch"]), 4), round(max(times["torch"]), 4)],
                      "targets_equal_torch_chain_and_wrapper_equal_launch": same, "mix_max_abs_diff_vs_torch_conv1d": float((m1 - m2).abs().max())}))


if __name__ == "__main__":
    main(sys.argv[1:])
