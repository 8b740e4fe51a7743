"""GPU: extended STOI (csrc/stoi.hip: k_stoi_corr_ext, fqss_stoi_x -> kernels.stoi(extended=) -> process) against the fp64 checker, the
cases and the gate of tests/test_estoi_cpu.py, on pitched rows.  Measured on an MI355X: S = 3.3e-16 (the floor of 1e-12 holds); grid and
silence cases at most 7.8e-16 from the checker, the frame-count cases 3.4e-14 (the checker's routes differ by 3.2e-14 there)."""
import numpy as np
import pytest
import torch

from tests import helpers_stoi as H
from tests.test_estoi_cpu import FRAME_RULE, check, estoi_rows, frame_case, grid, grid_case
from tests.test_gpu_stoi import pitched

pytestmark = pytest.mark.gpu
NAN = float("nan")


def gpu_estoi(est, ref, fs):
    from fqss_amd import kernels as K
    got = K.stoi(pitched(est), pitched(ref), fs, extended=True)
    assert got.dtype == torch.float64 and got.shape == (len(est),) and got.is_cuda
    return got.cpu().numpy()


def call_x(est, ref, fs, modes, stream=None):
    """fqss_stoi_x through the C ABI, the workspace and d NaN-filled: (status, d [popcount(modes)][P] as int64 on the host, ws, d's buffer)"""
    from fqss_amd import _lib
    from fqss_amd import kernels as K
    taps, up, down = K.stoi_taps(fs, est.device)
    (P, L), rows = est.shape, bin(modes & 3).count("1")
    need = _lib.query("fqss_stoi_x_ws_doubles", P, L, up, down, modes)
    ws = torch.full((_lib.query("fqss_stoi_x_ws_doubles", P, L, up, down, 3) + 64,), NAN, device="cuda", dtype=torch.float64)
    d = torch.full((2 * P + 2,), NAN, device="cuda", dtype=torch.float64)
    st = torch.cuda.current_stream() if stream is None else stream
    rc = _lib._bind("fqss_stoi_x")(est.data_ptr(), ref.data_ptr(), taps.data_ptr(), taps.numel(), ws.data_ptr(), need, d[1:].data_ptr(), P, L,
                                   est.stride(0), ref.stride(0), up, down, modes, st.cuda_stream)
    torch.cuda.synchronize()
    if rc == 0:
        assert bool(torch.isnan(ws[need:]).all()) and bool(torch.isnan(d[0])) and bool(torch.isnan(d[1 + rows * P:]).all()), "a guard was written"
    return rc, d[1:1 + rows * P].cpu().reshape(rows, P).view(torch.int64), ws, d


@pytest.mark.parametrize("fs", H.RATES)
def test_accuracy_grid_and_monotone_in_the_noise(fs):
    grid_case(gpu_estoi, fs)


@pytest.mark.parametrize("L,segments", FRAME_RULE)
def test_frame_counts_estimate_equal_to_reference_and_zero_estimate(L, segments):
    frame_case(gpu_estoi, L, segments)


@pytest.mark.parametrize("fs,silence", [(16000, ((0.35, 0.6),)), (8000, ((0.0, 0.1), (0.2, 0.3), (0.5, 0.55), (0.9, 1.0)))])
def test_segments_that_straddle_removed_frames(fs, silence):
    refs = np.stack([H.voiced(H.GRID_LENGTHS[fs], fs, 5 + i, silence=silence) for i in range(3)])
    ests = np.stack([H.noisy(r, 5.0, 6 + i) for i, r in enumerate(refs)])
    check(gpu_estoi(ests, refs, fs), estoi_rows(ests, refs, fs), grid(fs)[3], f"fs = {fs}, silence {silence}")


@pytest.mark.parametrize("fs", [8000, 10000])
def test_both_modes_are_the_bits_of_each_alone_again_and_on_a_side_stream(fs):
    from fqss_amd import kernels as K
    est, ref = pitched(grid(fs)[0]), pitched(grid(fs)[1])
    e0, r0 = est.clone(), ref.clone()
    rc, both, _, _ = call_x(est, ref, fs, 3)
    assert rc == 0 and torch.equal(both[0], K.stoi(est, ref, fs).cpu().view(torch.int64)), "row 0 is not fqss_stoi's d"
    for modes, rows in ((1, both[:1]), (2, both[1:]), (3, both)):
        assert torch.equal(call_x(est, ref, fs, modes)[1], rows), modes
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = call_x(est, ref, fs, 3, stream=side)[1]
        pair = torch.stack(K.stoi(est, ref, fs, extended="both"))
    side.synchronize()
    assert torch.equal(again, both) and torch.equal(pair.cpu().view(torch.int64), both), "d differs on another stream"
    assert torch.equal(est.view(torch.int32), e0.view(torch.int32)) and torch.equal(ref.view(torch.int32), r0.view(torch.int32))


@pytest.mark.parametrize("modes", [0, 4])
def test_modes_outside_1_to_3_are_refused_and_write_nothing(modes):
    from fqss_amd import _lib
    rc, _, ws, d = call_x(pitched(grid(8000)[0][:, :3000]), pitched(grid(8000)[1][:, :3000]), 8000, modes)
    assert rc == -22 and "fqss_stoi_x" in _lib.load().fqss_last_error().decode()      # FQSS_EINVAL
    assert bool(torch.isnan(d).all()) and bool(torch.isnan(ws).all()), "a refused call wrote"


def test_metric_evaluation_reports_estoi_of_the_matched_pairs_when_asked():
    from fqss_amd import process
    e, r, _, gate = grid(8000)
    ref_np = np.stack([r[0], H.voiced(7200, 8000, 99)])
    est_np = np.stack([H.noisy(ref_np[1], 5.0, 100), e[0]])                  # estimate 0 belongs to target 1 and the reverse
    est, clean = torch.from_numpy(est_np).cuda(), torch.from_numpy(ref_np).cuda()
    s0, d0, st0 = process.metric_evaluation(est, clean, sample_rate=8000, with_stoi=True)
    s1, d1, st1 = process.metric_evaluation(est, clean, sample_rate=8000, with_stoi=True, stoi_extended=True)
    assert (s1, d1) == (s0, d0) and st1 != st0
    want = estoi_rows(est_np, ref_np[::-1], 8000)
    check([st1], [want.mean()], gate, "metric_evaluation ESTOI")
    check(process.stoi(est[:, None], clean.flip(0)[:, None], 8000, extended=True).cpu().numpy(), want, gate, "process.stoi")
