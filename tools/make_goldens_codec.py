#!/usr/bin/env python
"""Writes tests/golden/codec_split.npz: the two-plane splitter of the reference's own process.preprocess (process.py:16-37) in both forms,
normalize=True and normalize=False, on inputs with values on bin edges (multiples of thr / 128), +-thr, +-0 and denormals, and row by row
(the per-item form: the reference calls the model on one chunk at a time).

Runs where the reference is importable (tools/ref_shim.py), like tools/make_goldens.py; the tests only read the file.

    python tools/make_goldens_codec.py [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: E402

ref_shim.install()

import torch  # noqa: E402

torch.set_num_threads(1)
sys.path.insert(0, ref_shim.REFERENCE_ROOT)
import process as RP  # noqa: E402


def inputs():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 96, generator=g) * 0.3 + 0.03
    x = x * torch.tensor([1.0, 1e-3, 7.0, 0.05])[:, None]
    for b in range(4):
        thr = float(x[b].abs().max()) * 1.25
        x[b, :12] = torch.tensor([thr, -thr, 0.0, -0.0, 1e-40, -1e-40, thr / 128, -thr / 128, 5 * thr / 128, thr * 127 / 128, thr / 256,
                                  77 * thr / 128])
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"))
    args = ap.parse_args()
    x = inputs()
    out = dict(x=x.numpy(),
               norm=RP.preprocess(x.clone(), n_splitter=2).numpy(),
               raw=RP.preprocess(x.clone(), n_splitter=2, normalize=False).numpy(),
               rows=torch.cat([RP.preprocess(x[b:b + 1].clone(), n_splitter=2) for b in range(4)]).numpy())
    np.savez(os.path.join(args.out, "codec_split.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
