"""GPU: short-time objective intelligibility (csrc/stoi.hip: fqss_stoi -> kernels.stoi -> process.stoi / metric_evaluation -> val.py)
against the fp64 checker of tests/helpers_stoi.py (the statement of include/fqss.h by other routes: the resampler as a full convolution,
the silent-frame removal as an overlap-add into a buffer, spectra through numpy.fft).

Gate: |GPU - checker| <= helpers_stoi.gate(S) = max(1e-12, 1000 S) on d, absolute, on every case of this file; S is the spread of the
checker's own two spectrum routes (rfft / DFT matrix) over the accuracy grid, measured here by the `grid` fixture (at most 7e-16 on
inputs of this kind, so the floor of 1e-12 is what holds).  Three decades cover the kernel's other FFT factorisation and summation
orders; a single fp32 intermediate would cost about 1e-7.  The gate does not come from the kernel.
Measured on an MI355X: S = 3.3e-16; accuracy grid max |GPU - checker| = 1.3e-15 (8 kHz; 2.2e-16 at 10 kHz, 0 at 16 kHz); the frame-rule,
silence and length cases at most 5.0e-15; est = ref within 2.2e-16 of 1.

Shapes.  0.9 s per rate (9000 / 7200 / 14400 samples: 69 frames at 10 kHz, about 50 kept) and lengths that are no multiple of `down`;
256 + 128 k and one more sample (the strict frame rule); 31 and 30 kept frames (one segment; none: 1e-5); L < 256.  The resampler's
tile is 256 outputs, the scan of k_stoi_mask takes 256 frames per round: 9000 samples are 36 tiles, one round; the 3.5 s case is two
rounds."""
import os
import re

import numpy as np
import pytest
import torch
import yaml

from tests import helpers_stoi as H

pytestmark = pytest.mark.gpu
EINVAL = -22
NAN = float("nan")
K = None
_lib = None


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    global K, _lib
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from fqss_amd import _lib as lib
    from fqss_amd import kernels
    K, _lib = kernels, lib
    yield


@pytest.fixture(scope="module")
def grid():
    """{fs: (est [3, L], ref [3, L], checker's d [3])} at 20 / 5 / -5 dB, and the gate from the spread of the checker's two routes"""
    out, spread = {}, 0.0
    for fs in H.RATES:
        cases = [H.grid_case(fs, snr) for snr in H.SNRS_DB]
        est, ref = np.stack([e for e, _ in cases]), np.stack([r for _, r in cases])
        want = H.stoi_ref_rows(est, ref, fs)
        spread = max(spread, np.abs(want - H.stoi_ref_rows(est, ref, fs, dft="matrix")).max())
        out[fs] = (est, ref, want)
    print(f"checker spread S = {spread:.3g}, gate = {H.gate(spread):.3g}")
    return out, H.gate(spread)


def pitched(rows, pad=13, off=5):
    """the rows as the middle columns of a larger NaN-filled device buffer: a read outside a row poisons the result"""
    rows = np.asarray(rows, dtype=np.float32)
    P, L = rows.shape
    buf = torch.full((P + 2, L + pad), NAN, device="cuda")
    view = buf[1:1 + P, off:off + L]
    view.copy_(torch.from_numpy(rows))
    return view


def call_stoi(est, ref, fs, ws=None, d=None, taps=None, n_taps=None, L=None, ld_e=None, ld_r=None, n_ws=None, P=None, up=None, down=None,
              stream=None, null=()):
    """fqss_stoi through the C ABI with a NaN-filled workspace: (status, message, d)"""
    tp, p, q = K.stoi_taps(fs, est.device)
    taps = tp if taps is None else taps
    P_, L_ = est.shape
    up, down = p if up is None else up, q if down is None else down
    need = _lib.query("fqss_stoi_ws_doubles", P_, L_, p, q)
    ws = torch.full((need + 64,), NAN, device="cuda", dtype=torch.float64) if ws is None else ws
    d = torch.full((P_ + 2,), NAN, device="cuda", dtype=torch.float64) if d is None else d
    ptr = dict(est=est.data_ptr(), ref=ref.data_ptr(), taps=taps.data_ptr(), ws=ws.data_ptr(), d=d[1:].data_ptr())
    for name in null:
        ptr[name] = None
    st = torch.cuda.current_stream() if stream is None else stream
    rc = _lib._bind("fqss_stoi")(ptr["est"], ptr["ref"], ptr["taps"], taps.numel() if n_taps is None else n_taps, ptr["ws"],
                                 need if n_ws is None else n_ws, ptr["d"], P_ if P is None else P, L_ if L is None else L,
                                 est.stride(0) if ld_e is None else ld_e, ref.stride(0) if ld_r is None else ld_r, up, down, st.cuda_stream)
    msg = _lib.load().fqss_last_error().decode()
    torch.cuda.synchronize()
    if rc == 0:
        assert bool(torch.isnan(ws[need:]).all()), "a workspace guard was written"
        assert bool(torch.isnan(d[0])) and bool(torch.isnan(d[P_ + 1:]).all())
    return rc, msg, d[1:1 + P_].cpu()


def gpu_stoi(est, ref, fs):
    """kernels.stoi and the raw C ABI (NaN-filled workspace) on pitched rows; both must be the same bits"""
    e, r = pitched(est), pitched(ref)
    got = K.stoi(e, r, fs)
    assert got.dtype == torch.float64 and got.shape == (len(est),) and got.is_cuda
    rc, msg, raw = call_stoi(e, r, fs)
    assert rc == 0, msg
    assert torch.equal(got.cpu().view(torch.int64), raw.view(torch.int64)), "kernels.stoi and the C ABI differ"
    return got.cpu().numpy()


def check(got, want, gate, what):
    err = np.abs(np.asarray(got) - np.asarray(want)).max()
    print(f"{what}: max |GPU - checker| = {err:.3g}")
    assert np.isfinite(got).all() and err <= gate, (what, got, want)


def test_accuracy_grid_and_monotone_in_the_noise(grid):
    cases, gate = grid
    for fs, (est, ref, want) in cases.items():
        got = gpu_stoi(est, ref, fs)
        check(got, want, gate, f"grid fs = {fs}")
        assert got[0] > got[1] > got[2] and 0.5 < got[2] and got[0] < 0.999, got


def test_estimate_equal_to_reference_is_one(grid):
    cases, gate = grid
    for fs, (est, ref, _) in cases.items():
        got = gpu_stoi(ref[:1], ref[:1], fs)
        assert abs(got[0] - 1.0) <= gate, (fs, got)
        check(got, [H.stoi_ref(ref[0], ref[0], fs)], gate, f"est = ref, fs = {fs}")


@pytest.mark.parametrize("fs,L", [(8000, 7203), (8000, 7201), (16000, 14405), (16000, 14403)])
def test_lengths_that_are_no_multiple_of_down(grid, fs, L):
    _, gate = grid
    est, ref = H.grid_case(fs, 5.0, L)
    check(gpu_stoi(est[None], ref[None], fs), [H.stoi_ref(est, ref, fs)], gate, f"fs = {fs}, L = {L}")


@pytest.mark.parametrize("L,frames", [(256 + 128 * 34, 34), (256 + 128 * 34 + 1, 35), (256 + 128 * 30 + 1, 31), (256 + 128 * 30, 30)])
def test_strict_frame_rule_one_segment_and_too_few_frames(grid, L, frames):
    """10 kHz, no silent stretch: every frame is kept.  L' = 256 + 128 k drops the frame that ends at the last sample; 31 kept frames are
    one segment, 30 are none: d == 1e-5 exactly"""
    _, gate = grid
    ref = H.voiced(L, 10000, 77, silence=())
    est = H.noisy(ref, 5.0, 78)
    want, kept, margin = H.stoi_ref(est, ref, 10000, want_info=True)
    assert kept == frames and margin >= 0.1, (kept, margin)
    got = gpu_stoi(est[None], ref[None], 10000)
    if frames == 30:
        assert want == 1e-5 and got[0] == 1e-5, (got, want)
    else:
        assert want != 1e-5
        check(got, [want], gate, f"L = {L}: {frames} frames")


@pytest.mark.parametrize("fs,silence", [(8000, ((0.0, 0.22),)), (8000, ((0.8, 1.0),)), (16000, ((0.35, 0.6),)), (8000, ()),
                                        (8000, ((0.0, 0.1), (0.2, 0.3), (0.5, 0.55), (0.9, 1.0)))])
def test_silence_at_the_start_the_end_the_middle_and_none(grid, fs, silence):
    _, gate = grid
    L = H.GRID_LENGTHS[fs]
    ref = H.voiced(L, fs, 5, silence=silence)
    est = H.noisy(ref, 5.0, 6)
    want, kept, margin = H.stoi_ref(est, ref, fs, want_info=True)
    assert margin >= 0.1 and (kept == 69) == (silence == ()), (kept, margin)
    check(gpu_stoi(est[None], ref[None], fs), [want], gate, f"fs = {fs}, silence {silence}: {kept} of 69 frames")


def test_exactly_31_and_30_kept_frames_out_of_more(grid):
    """8 kHz with a silent tail: the kept frames are counted by the checker, the lengths chosen so that 31 / 30 are left"""
    _, gate = grid
    found = {}
    for L in range(4100, 4400, 8):
        ref = H.voiced(L, 8000, 9, silence=((0.72, 1.0),))
        _, kept, margin = H.stoi_ref(ref, ref, 8000, want_info=True)
        if kept in (30, 31) and kept not in found and margin >= 0.1:
            found[kept] = ref
        if len(found) == 2:
            break
    assert sorted(found) == [30, 31], sorted(found)
    for kept, ref in found.items():
        est = H.noisy(ref, 5.0, 10)
        want = H.stoi_ref(est, ref, 8000)
        got = gpu_stoi(est[None], ref[None], 8000)
        if kept == 30:
            assert want == 1e-5 and got[0] == 1e-5, got
        else:
            check(got, [want], gate, "31 kept frames of more")


def test_more_frames_than_one_scan_round(grid):
    """3.5 s at 16 kHz: 272 frames, the kept-frame scan of k_stoi_mask takes two rounds of 256"""
    _, gate = grid
    L = 56000
    ref = H.voiced(L, 16000, 21)
    est = H.noisy(ref, 5.0, 22)
    want, kept, margin = H.stoi_ref(est, ref, 16000, want_info=True)
    assert margin >= 0.1 and kept > 150, (kept, margin)
    check(gpu_stoi(est[None], ref[None], 16000), [want], gate, f"L = {L}: {kept} frames kept")


@pytest.mark.parametrize("fs,L", [(10000, 200), (10000, 256), (8000, 200), (16000, 1), (10000, 257)])
def test_short_inputs_give_1e_minus_5(fs, L):
    ref = H.voiced(max(L, 32), fs, 3, silence=())[:L]
    got = gpu_stoi(np.stack([ref, ref]), np.stack([ref, ref]), fs)
    assert (got == 1e-5).all(), got


def test_all_zero_reference_is_the_checkers_finite_value(grid):
    cases, gate = grid
    for fs in H.RATES:
        est = cases[fs][0][:1]
        ref = np.zeros_like(est)
        want = H.stoi_ref(est[0], ref[0], fs)
        assert np.isfinite(want)
        check(gpu_stoi(est, ref, fs), [want], gate, f"zero reference, fs = {fs}")


def test_same_bits_twice_and_on_another_stream_inputs_unchanged(grid):
    cases, _ = grid
    for fs in (8000, 10000):
        est, ref = pitched(cases[fs][0]), pitched(cases[fs][1])
        e0, r0 = est.clone(), ref.clone()
        rc, msg, first = call_stoi(est, ref, fs)
        assert rc == 0, msg
        rc, msg, second = call_stoi(est, ref, fs)
        assert rc == 0 and torch.equal(first.view(torch.int64), second.view(torch.int64)), "d differs between two runs"
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            rc, msg, third = call_stoi(est, ref, fs, stream=side)
            via_kernels = K.stoi(est, ref, fs)
        side.synchronize()
        assert rc == 0 and torch.equal(first.view(torch.int64), third.view(torch.int64)), "d differs on another stream"
        assert torch.equal(first.view(torch.int64), via_kernels.cpu().view(torch.int64))
        assert torch.equal(est.view(torch.int32), e0.view(torch.int32)) and torch.equal(ref.view(torch.int32), r0.view(torch.int32))


def test_out_of_contract_arguments_are_refused_and_write_nothing(grid):
    cases, _ = grid
    est, ref = pitched(cases[8000][0][:, :3000]), pitched(cases[8000][1][:, :3000])
    need = _lib.query("fqss_stoi_ws_doubles", 3, 3000, 5, 4)
    assert need > 0
    ws = torch.full((need + 64,), NAN, device="cuda", dtype=torch.float64)
    d = torch.full((5,), NAN, device="cuda", dtype=torch.float64)
    even = torch.ones(364, device="cuda", dtype=torch.float64)
    bad = [dict(P=0), dict(L=0), dict(L=-3), dict(ld_e=2999), dict(ld_r=2999), dict(n_ws=need - 1), dict(up=10, down=8), dict(up=0), dict(down=0),
           dict(up=-5), dict(taps=even, n_taps=364), dict(n_taps=0), dict(up=1, down=1), dict(null=("est",)), dict(null=("ref",)),
           dict(null=("taps",)), dict(null=("ws",)), dict(null=("d",))]
    for kw in bad:
        rc, msg, _ = call_stoi(est, ref, 8000, ws=ws, d=d, **kw)
        assert rc == EINVAL and "fqss_stoi" in msg, (kw, rc, msg)
    assert bool(torch.isnan(d).all()) and bool(torch.isnan(ws).all()), "a refused call wrote"
    for args in ((0, 3000, 5, 4), (3, 0, 5, 4), (3, 3000, 10, 8), (3, 3000, 0, 4), (3, 3000, 5, 0)):
        assert _lib.query("fqss_stoi_ws_doubles", *args) == 0, args
    with pytest.raises(NotImplementedError, match="44100"):
        K.stoi(est, ref, 44100)


def test_metric_evaluation_reports_stoi_of_the_matched_pairs_when_asked(grid):
    """two estimates swapped against the targets: the STOI slot is the checker's mean over the SI-SNR-matched pairs at the rate given,
    NaN by default, and the other two slots do not change"""
    from fqss_amd import process
    cases, gate = grid
    est_np, ref_np = cases[8000][0][:2], np.stack([cases[8000][1][0], H.voiced(7200, 8000, 99)])
    est_np = np.stack([H.noisy(ref_np[1], 5.0, 100), est_np[0]])                  # estimate 0 belongs to target 1 and the reverse
    est, clean = torch.from_numpy(est_np).cuda(), torch.from_numpy(ref_np).cuda()
    match = K.sisnr_matrix(est, clean).argmax(dim=1).cpu().numpy()
    assert list(match) == [1, 0]
    s0, d0, st0 = process.metric_evaluation(est, clean)
    assert np.isnan(st0) and np.isfinite(d0)
    for fs in (8000, 16000):
        s1, d1, st1 = process.metric_evaluation(est, clean, sample_rate=fs, with_stoi=True)
        assert (s1, d1) == (s0, d0) and isinstance(st1, float)
        check([st1], [np.mean([H.stoi_ref(est_np[p], ref_np[match[p]], fs) for p in range(2)])], gate, f"metric_evaluation STOI at {fs}")
    s2, d2, st2 = process.metric_evaluation(est, clean, sample_rate=8000, with_sdr=False, with_stoi=True)
    assert s2 == s0 and np.isnan(d2) and st2 == process.metric_evaluation(est, clean, sample_rate=8000, with_stoi=True)[2]
    got = process.stoi(est.reshape(2, 1, -1), clean.flip(0).reshape(2, 1, -1), 8000)
    assert got.is_cuda and got.shape == (2,)
    check(got.cpu().numpy(), [H.stoi_ref(est_np[p], ref_np[1 - p], 8000) for p in range(2)], gate, "process.stoi")


def test_val_cli_prints_stoi_when_the_config_asks(tmp_path, capsys):
    """`val.py -y cfg.yaml` on synthetic mixtures with testing_cfg.stoi: true: the last line carries STOI=<the checker's mean over the
    items, three decimals>; without the key it still ends in STOI=nan; val() returns two values either way"""
    from fqss_amd import process
    from fqss_amd import val as V
    from fqss_amd.data import synth_batch
    from fqss_amd.quantization.qat.models.load_model import create_pretrained_model, enable_observer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    conf = yaml.safe_load(open(os.path.join(root, "configs", "convtasnet_2spks_8k_synthetic.yaml")))
    ckpt = tmp_path / "best_model.pth"
    torch.save(create_pretrained_model(dict(conf["model_cfg"], model_path=None)).state_dict(), ckpt)
    conf["model_cfg"]["model_path"] = str(ckpt)
    testing = dict(n_items=2, length_samples=12000, segment_samples=8000, overlap=0.25)
    lines = {}
    for key in (True, None):
        conf["testing_cfg"] = dict(testing, stoi=True) if key else dict(testing, n_items=1)
        yml = tmp_path / f"val_{key}.yaml"
        yml.write_text(yaml.safe_dump(conf))
        capsys.readouterr()
        out = V.val(["-y", str(yml)])
        assert isinstance(out, tuple) and len(out) == 2 and all(np.isfinite(out))
        lines[key] = capsys.readouterr().out.strip().splitlines()[-1]
    assert re.fullmatch(r"SI-SDR=(-?\d+\.\d\d),SI-SDR-imp=(-?\d+\.\d\d),SDR=(-?\d+\.\d\d),STOI=nan", lines[None]), lines[None]
    m = re.fullmatch(r"SI-SDR=(-?\d+\.\d\d),SI-SDR-imp=(-?\d+\.\d\d),SDR=(-?\d+\.\d\d),STOI=(\d\.\d{3})", lines[True])
    assert m, lines[True]
    # the same estimates again, through the checker
    model = create_pretrained_model(conf["model_cfg"])
    enable_observer(model, False)
    model.to("cuda").eval()
    want = []
    for i in range(2):
        mix, clean = synth_batch(1, 12000, seed=10_000 + i, device="cuda")
        wavs = process.model_infer(model, mix[0], n_srcs=2, segment=8000, overlap=0.25, device="cuda", target=clean[0])
        match = K.sisnr_matrix(wavs.reshape(2, -1), clean[0]).argmax(dim=1).cpu().numpy()
        w, c = wavs.reshape(2, -1).cpu().numpy(), clean[0].cpu().numpy()
        want.append(np.mean([H.stoi_ref(w[p], c[match[p]], 8000) for p in range(2)]))
    print(f"val.py STOI line {m.group(4)}, checker {np.mean(want):.6f}")
    assert abs(float(m.group(4)) - np.mean(want)) <= 5e-4, (lines[True], want)
