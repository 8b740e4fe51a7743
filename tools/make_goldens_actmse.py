#!/usr/bin/env python3
"""Golden ranges of the histogram-MSE activation observer from the REAL reference's GradientActivationFakeQuantize_MSE
(qat_quant.py:245-326), through tools/ref_shim.py (build container only).  50 seeded tensors of 2048 values -- Gaussians of growing
scale, every other one ReLU-shifted, one large outlier each -- are fed to the reference's class; call 51 runs its search.  Written to
tests/golden/act_mse.npz: the inputs `x` [50, 2048] fp32 and `range` = (min_range, max_range) fp32 [2] (data only).

The outliers are multiples of 0.25, and that is a condition on the inputs: the narrowest tensor is then a post-ReLU one over [0, 4.75],
whose bin width 4.75 / 512 is exact in fp32, so the reference's `bins[1] - bins[0]` on numpy's fp32 edges is the fp64 width of
include/fqss.h and both statements walk the same merged grid (7400 points; 12 of 12 seeds then agree to the last bit).  With a width
that fp32 rounds -- outliers not on such a grid -- the reference's merged grid drifts by more than a bin over its length (measured: its far
end, and with it max_range, moves by 2e-4 of the span) and, the error table being rough (the merged grid beats against the 255 levels:
scattered (i, j) within 0.1 % of the minimum), the two statements pick different winners on 20 of 24 seeds.  main() asserts that the fp64
statement (tests/helpers_aq_mse.py) reproduces the reference's pair within the fixture's gate.
Usage: python tools/make_goldens_actmse.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: E402

ref_shim.install()

import torch  # noqa: E402

from quantization.qat import qat_quant as RQ  # noqa: E402

N_OBS, N_VALUES = 50, 2048


SEED = 1


def inputs(seed=SEED):
    rng = np.random.default_rng(seed)
    xs = np.empty((N_OBS, N_VALUES), dtype=np.float32)
    for t in range(N_OBS):
        x = rng.standard_normal(N_VALUES) * (0.5 + 0.03 * t)
        if t % 2:
            x = np.maximum(x + 0.3, 0.0)                     # a post-ReLU activation: half its values in one bin
        x[rng.integers(N_VALUES)] = np.round((9.0 + 0.2 * t) * (0.5 + 0.03 * t) * 4) / 4 * (1.0 if t % 4 < 3 else -1.0)      # one click per utterance
        xs[t] = x.astype(np.float32)
    return xs


def main():
    xs = inputs()
    q = RQ.GradientActivationFakeQuantize_MSE(True).to(RQ.DEVICE)
    with torch.no_grad():
        for t in range(N_OBS):
            q(torch.from_numpy(xs[t]).to(RQ.DEVICE))
        assert q.observer_mode and float(q.min_range) == -0.5
        q(torch.from_numpy(xs[0]).to(RQ.DEVICE))             # call 51: merge_hist + mse_minmax_range
    assert not q.observer_mode
    rng_ = np.array([float(q.min_range.detach()), float(q.max_range.detach())], dtype=np.float32)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from tests import helpers_aq_mse as H
    chk = H.search(*H.rows_for(list(xs)))
    assert chk["gap"] > 1e-6 and max(abs(float(chk["mn"]) - rng_[0]), abs(float(chk["mx"]) - rng_[1])) <= 1e-5 * chk["span"], \
        (chk["i"], chk["j"], chk["gap"], chk["mn"], chk["mx"], rng_)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "act_mse.npz")
    np.savez_compressed(out, x=xs, range=rng_)
    print("act_mse:", xs.shape, "range", rng_, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
