"""`kernels.hd_repitch` (fqss_hd_repitch, csrc/repitch.hip) against its statement in include/fqss.h, restated in NumPy int64
(tests/helpers_repitch.py).  The statement is integer, so the output AND the segment positions are compared with torch.equal."""
import numpy as np
import pytest
import torch

from tests.helpers_repitch import J, repitch_batch

pytestmark = pytest.mark.gpu

T_IN, T_RP = 12000, 10560            # int((1 - 0.12) * 12000): about 8 segments of 1536


def streams(C):
    rng = np.random.default_rng(5)
    noise = np.cumsum(rng.standard_normal((2, T_IN + 8, C)), axis=1)
    noise = noise[:, 8:] - noise[:, :-8]                                             # an 8-sample moving sum: low-passed
    noise = np.rint(noise / noise.std() * 8192).clip(-32768, 32767)                  # about -12 dBFS
    period = np.rint(9000 * rng.standard_normal((147, C))).clip(-32768, 32767)
    periodic = np.tile(period, (T_IN // 147 + 1, 1))[:T_IN]                          # exact cost ties 147 samples apart
    square = np.where((np.arange(T_IN) // 37) % 2 == 0, 32767, -32767)[:, None].repeat(C, axis=1)
    square[1::2, -1] = -32768                                                        # the most negative code too
    tail = noise[1].copy()
    tail[2 * T_IN // 3:] = 0                                                         # the end of a track
    out = dict(noise=noise[0], periodic=periodic, zeros=np.zeros((T_IN, C)), square=square, tail=tail)
    return {k: v.astype(np.int16) for k, v in out.items()}


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("pitch,tempo", [(0, 12.0), (0, -12.0), (1, 0.0), (-2, 7.3), (2, -12.0)])
def test_repitch_is_the_statement_bit_for_bit(C, pitch, tempo):
    from fqss_amd import kernels as K
    x = streams(C)
    A = K.repitch_A(pitch, tempo)
    for names, on in ((("noise", "periodic", "zeros", "noise"), (1, 1, 1, 0)), (("square", "tail", "periodic", "noise"), (1, 1, 0, 1))):
        pcm = np.stack([x[n] for n in names]).reshape(2, 2, T_IN, C)
        on_t = torch.tensor(on).reshape(2, 2)
        rows = (on_t, torch.full((2, 2), pitch) * on_t, torch.full((2, 2), A))
        want, want_pos = repitch_batch(pcm, T_RP, *(r.numpy() for r in rows), K.REPITCH_RATIOS, K.repitch_taps)
        got, pos = K.hd_repitch(torch.from_numpy(pcm).cuda(), T_RP, *rows, return_pos=True)
        assert got.dtype == torch.int16 and torch.equal(pos.cpu(), torch.from_numpy(want_pos)), names
        assert torch.equal(got.cpu(), torch.from_numpy(want)), names
        if "zeros" in names:                                   # all costs tie: the lowest offset, and silence stays silence
            P, Q = K.REPITCH_RATIOS[pitch]
            m = np.arange(1, (((T_RP - 1) * P) // Q + J // 2) // 1536 + 1)
            assert want_pos[1, 0, m].tolist() == (((m * 1536 * A) >> 16) - 512).tolist() and not want[1, 0].any()


@pytest.mark.parametrize("C,pitch,tempo", [(2, 1, 0.0), (1, -2, -5.0)])
def test_a_constant_stays_the_constant(C, pitch, tempo):
    """every phase's taps sum to exactly 2^15, so PCM 1000 comes back as 1000 behind the ramp over the zeros below index 0"""
    from fqss_amd import kernels as K
    pcm = torch.full((1, 2, T_IN, C), 1000, dtype=torch.int16)
    one = torch.ones(1, 2, dtype=torch.int64)
    got = K.hd_repitch(pcm.cuda(), T_RP, one, pitch * one, K.repitch_A(pitch, tempo) * one).cpu()
    assert bool((got[:, :, J:] == 1000).all()) and int(got[0, 0, 0, 0]) != 1000
