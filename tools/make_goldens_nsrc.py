#!/usr/bin/env python
"""Writes tests/golden/nsrc_loss.npz: the three-source KD objective of the asteroid env (mysystem.py:124-151) from the reference's own
wsdr.py (`pairwise_wsisdr`, `PairwiseWSDR("sisdr", take_log=True)`) and the restated asteroid PIT of tools/make_goldens.py, in fp64.

Runs where the reference is importable (tools/ref_shim.py), like tools/make_goldens.py; the tests only read the file.

The batch holds one sample per permutation of three sources, B = 6, S = 3, T = 1000:
    perms = list(itertools.permutations(range(3)))
    s    = 0.05 randn(6, 3, T)                            seed 1
    e[b] = s[b, perms[b]]           + 0.3 * 0.05 randn    seed 10 + b
    f[b] = s[b, perms[(5b+2) % 6]]  + 0.2 * 0.05 randn    seed 20 + b
so the student's best permutation differs in every sample, the teacher's is a different one again, and the two samples built with a
3-cycle select the OTHER 3-cycle (a PIT candidate is mean_i pw[est = p[i]][tgt = i]: e = s[p] puts target p[i] on estimate i, which
p's inverse undoes).  A loss that mixes up p and its inverse passes every two-source test and fails on those two samples.

    python tools/make_goldens_nsrc.py [--out tests/golden]
"""
import argparse
import importlib.util
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: E402

ref_shim.install()

import torch  # noqa: E402

torch.set_num_threads(1)

_spec = importlib.util.spec_from_file_location("ref_wsdr", os.path.join(ref_shim.REFERENCE_ROOT, "train_env/asteroid_librimix/wsdr.py"))
RW = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(RW)

EPS = 1e-8
PERMS = list(itertools.permutations(range(3)))
_pw_log = RW.PairwiseWSDR("sisdr", take_log=True)


def candidates(pw):
    """asteroid PITLossWrapper(pit_from='pw_mtx') restated: pw[b, est_i, tgt_j] -> [b, n_perms] of mean_i pw[b, p[i], i]"""
    n = pw.shape[-1]
    return torch.stack([sum(pw[:, p[i], i] for i in range(n)) / n for p in itertools.permutations(range(n))], dim=1)


def pit_min_mean(pw):
    return torch.mean(torch.min(candidates(pw), dim=1)[0])


def common_step(est, fest, targets, kd_lambda=0.1):
    """mysystem.py:124-151 around the reference's wsdr code (tools/make_goldens.py::common_step without the models)"""
    with torch.no_grad():
        sdrs = torch.stack([pit_min_mean(-_pw_log(fest[b:b + 1], targets[b:b + 1])) for b in range(len(fest))])
        sdrqs = torch.stack([pit_min_mean(-_pw_log(est[b:b + 1].detach(), targets[b:b + 1])) for b in range(len(fest))])
        w = 10 ** ((sdrs - sdrqs) / 10)
    kd = -pit_min_mean(RW.pairwise_wsisdr(est, fest, weights=w))
    task = -pit_min_mean(RW.pairwise_wsisdr(est, targets))
    loss = -10 * torch.log10((1 - kd_lambda) * task + kd_lambda * kd + EPS)
    return loss, kd, task, w, sdrs, sdrqs


def inputs(B=6, T=1000):
    """the batch of the docstring; B > 6 repeats the six-sample pattern with fresh noise (tests/test_gpu_nsrc.py builds the same)"""
    s = 0.05 * torch.randn(B, 3, T, generator=torch.Generator().manual_seed(1))
    e, f = torch.empty_like(s), torch.empty_like(s)
    for b in range(B):
        e[b] = s[b, list(PERMS[b % 6])] + 0.3 * 0.05 * torch.randn(3, T, generator=torch.Generator().manual_seed(10 + b))
        f[b] = s[b, list(PERMS[(5 * b + 2) % 6])] + 0.2 * 0.05 * torch.randn(3, T, generator=torch.Generator().manual_seed(20 + b))
    return s, e, f


def check_design(s, e, f, min_margin_db):
    """every permutation is selected once, with a clear margin; the 3-cycle samples select the inverse 3-cycle"""
    c = candidates(-_pw_log(e.double(), s.double()))
    best = c.argmin(dim=1).tolist()
    assert sorted(best[:6]) == list(range(6)), best
    for b in range(len(best)):
        p = PERMS[b % 6]
        inv = tuple(p.index(i) for i in range(3))
        assert PERMS[best[b]] == inv, (b, p, PERMS[best[b]])
    assert PERMS[best[3]] == PERMS[4] and PERMS[best[4]] == PERMS[3]          # the two 3-cycles: each selects the other
    top2 = c.topk(2, dim=1, largest=False)[0]
    margin = float((top2[:, 1] - top2[:, 0]).min())
    assert margin >= min_margin_db, margin
    return margin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"))
    args = ap.parse_args()
    s, e, f = inputs()
    print("margin to the runner-up at T = 1000: %.1f dB" % check_design(s, e, f, 24.0))
    print("margin to the runner-up at T = 16389: %.1f dB" % check_design(*inputs(6, 16389), 32.0))
    r32 = common_step(e, f, s)
    e64 = e.double().requires_grad_(True)
    loss, kd, task, w, sdrs, sdrqs = common_step(e64, f.double(), s.double())
    for a, b in zip(r32[:3], (loss, kd, task)):
        assert abs(float(a.detach()) - float(b.detach())) <= 1e-7 * abs(float(b.detach()))
    loss.backward()
    npy = lambda t: t.detach().numpy().copy()
    path = os.path.join(args.out, "nsrc_loss.npz")
    np.savez_compressed(path, tgt=npy(s), est=npy(e), fest=npy(f), loss=npy(loss), kd=npy(kd), task=npy(task), w=npy(w), sdrs=npy(sdrs),
                        sdrqs=npy(sdrqs), gest=npy(e64.grad))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
