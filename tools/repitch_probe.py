"""The repitch kernels of the htdemucs env (kernels.hd_repitch: k_rp_search, the sequential WSOLA search, and k_rp_resample, the rate
change) at the recipe's shape: B = 4 items x S = 4 stems of 10 s stereo at 44.1 kHz, cut to T_rp = 388080.  One device, one run: device
events around each stage launched alone (rows, taps and positions on the device already), warmed up, median of 20 repeats, with every
row on (pitch +2, tempo -12: the most segments) and with one row on (what `proba` 0.2 mostly draws: the search is one workgroup, the
other rows are copied).  Prints one JSON line; the bytes are what the rate change has to move (pcm read once, out written once).
    python tools/repitch_probe.py [B] [S] [seconds]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fqss_amd import _lib, kernels as K  # noqa: E402

SR, C, REPEATS, WARMUP = 44100, 2, 20, 3


def main(argv):
    assert torch.cuda.is_available(), "the probe measures on a ROCm device"
    B, S = (int(argv[0]) if argv else 4), (int(argv[1]) if len(argv) > 1 else 4)
    T_in = int(SR * (float(argv[2]) if len(argv) > 2 else 10.0))
    T_rp = int((1 - 0.12) * T_in)
    g = torch.Generator().manual_seed(0)
    walk = torch.cumsum(torch.randn(B, S, T_in, C, generator=g) * 200, dim=2)
    pcm = (walk - walk.mean(dim=2, keepdim=True)).clamp_(-32768, 32767).to(torch.int16).cuda()
    hq = K.repitch_table().cuda()
    M = _lib.query("fqss_hd_repitch_ws_bytes", B, S, T_rp) // (4 * B * S)
    pos = torch.zeros(B, S, M, dtype=torch.int32, device="cuda")
    out = torch.empty(B, S, T_rp, C, dtype=torch.int16, device="cuda")
    result = {"shape": {"B": B, "S": S, "C": C, "T_in": T_in, "T_rp": T_rp, "segments": M}}
    for label, n_on in (("all_on", B * S), ("one_on", 1)):
        on = torch.zeros(B * S, dtype=torch.int64)
        on[:n_on] = 1
        pitch, A = 2 * on, torch.full((B * S,), K.repitch_A(2, -12.0))
        K.check_repitch_rows(B, S, C, T_in, T_rp, on, pitch, A)
        rows = torch.stack([on, pitch + 2, A], dim=1).to(torch.int32).cuda()

        def launch(stages):
            _lib.call("fqss_hd_repitch", pcm.data_ptr(), rows.data_ptr(), hq.data_ptr(), pos.data_ptr(), out.data_ptr(), B, S, C, T_in, T_rp,
                      stages, torch.cuda.current_stream().cuda_stream)

        times = {"search": [], "resample": []}
        for i in range(WARMUP + REPEATS):
            for name, stages in (("search", _lib.CONSTANTS["FQSS_RP_SEARCH"]), ("resample", _lib.CONSTANTS["FQSS_RP_RESAMPLE"])):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch(stages)
                b.record()
                b.synchronize()
                if i >= WARMUP:
                    times[name].append(a.elapsed_time(b))
        same = torch.equal(out, K.hd_repitch(pcm, T_rp, on.view(B, S), pitch.view(B, S), A.view(B, S)))
        nbytes = 2 * C * B * S * (T_in + T_rp)
        t_s, t_r = statistics.median(times["search"]), statistics.median(times["resample"])
        result[label] = {"k_rp_search_ms": round(t_s, 3), "k_rp_search_ms_min_max": [round(min(times["search"]), 3), round(max(times["search"]), 3)],
                         "k_rp_resample_ms": round(t_r, 3), "k_rp_resample_ms_min_max": [round(min(times["resample"]), 3), round(max(times["resample"]), 3)],
                         "resample_GBps": round(nbytes / t_r / 1e6, 1), "stages_equal_wrapper": bool(same)}
    print(json.dumps(result))


if __name__ == "__main__":
    main(sys.argv[1:])
