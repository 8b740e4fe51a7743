"""Host side of the Sepformer recipe's `wavedrop` (kernels.notch_taps, prepare_data.draw_wavedrop): the composed notch filter and the
draws of TimeDomainSpecAugment from the global torch RNG, in the package's order.  No device is needed."""
import numpy as np
import pytest
import torch

from fqss_amd import kernels as K
from fqss_amd.train_env.speechbrain_librimix.prepare_data import draw_wavedrop, wavedrop_config


def test_notch_taps():
    delta = K.notch_taps([])
    assert delta.shape == (101,) and delta[50] == 1.0 and np.count_nonzero(delta) == 1
    h = K.notch_taps([0.2, 0.55, 0.9])
    assert h.shape == (101,) and h.dtype == np.float64 and np.array_equal(h, h[::-1]) and np.isfinite(h).all()
    assert abs(K.notch_taps([0.3]).sum() - 1.0) < 1e-12             # a notch has unit gain at DC: hlpf sums to 1, hhpf to 0


@pytest.mark.parametrize("prob", [1.0, 0.0], ids=["all_drawn", "gates_alone"])
def test_draws_stay_in_range_and_follow_the_stated_order(prob):
    """the same stream drawn here call by call; with both probabilities 0 that is the three gate draws and nothing else"""
    cfg, n, rel = wavedrop_config({"perturb_prob": 0.0, "drop_freq_prob": prob, "drop_chunk_prob": prob}), 20000, [1.0, 0.5, 0.03]
    for seed in range(20):
        torch.manual_seed(seed)
        freqs, chunks = draw_wavedrop(cfg, n, rel)
        state = torch.get_rng_state()
        assert len(freqs) <= 3 and all(1e-14 <= f <= 1.0 for f in freqs) and len(chunks) == 3
        for row, r in zip(chunks, rel):
            assert len(row) <= 5 <= K.SB_C_MAX and all(0 <= lo <= hi <= n and hi - lo <= 2000 and lo <= int(r * n) for lo, hi in row)
        torch.manual_seed(seed)
        torch.rand(1)                                                # the speed gate
        want_f, want_c = [], [[], [], []]
        if not float(torch.rand(1)) > prob:
            want_f = (torch.rand(int(torch.randint(0, 4, (1,)))) * (1 - 1e-14) + 1e-14).tolist()
        if not float(torch.rand(1)) > prob:
            times = torch.randint(0, 6, (3,))
            for b in (b for b in range(3) if times[b]):
                length = torch.randint(1000, 2001, (int(times[b]),))
                lo = torch.randint(0, max(0, int(rel[b] * n) - int(length.max())) + 1, (int(times[b]),))
                want_c[b] = [(int(x), min(int(x) + int(y), n)) for x, y in zip(lo, length)]
        assert (freqs, chunks) == (want_f, want_c) and torch.equal(torch.get_rng_state(), state)
        assert prob or (freqs, chunks) == ([], [[], [], []])
