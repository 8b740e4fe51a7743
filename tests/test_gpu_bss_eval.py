"""GPU: BSS-eval SDR / SIR / SAR (csrc/bss_eval.hip: fqss_bss_eval -> kernels.bss_eval -> process.bss_eval -> val.py) against the fp64
checker of tests/helpers_bss.py (the statement of include/fqss.h by another route: the explicit lagged-reference matrix and least
squares on it; a second route through the explicit normal equations gives the checker's own spread U per value).

Gate per value: max(1e-6 dB, 1000 U) (helpers_bss.check: fqss_sdr's floor, the STOI tests' factor).  Every case prints its figures.

Shapes.  PANEL = 32 columns per panel of the factorisation (kBssNB), 64 x 64 tiles in the trailing update, 512 time samples per
workgroup of the correlation kernel (kBssTile).  T = 4 keeps n = S T below one panel, T = 16 puts it on a panel edge at S = 2,
T = 11 gives n = 33 at S = 3 (one column past it), T = 40 spans several panels and, at S = 3, two update tiles; L = 500 lies inside one
correlation tile, 1000 and 2500 cross tile edges.  One full-size case: S = 3, T = 512, L = 8000 (order 1536, 48 panels)."""
import os

import numpy as np
import pytest
import torch
import yaml

from tests import helpers_bss as H

pytestmark = pytest.mark.gpu
PANEL, SHAPES = H.PANEL, H.SHAPES
_cases = {}


def case(S, T, L):
    """(est, ref, checker's [3, S], U [3, S]) computed once per shape"""
    if (S, T, L) not in _cases:
        est, ref = H.make_case(S, L, seed=100 * S + T)
        _cases[S, T, L] = (est, ref) + H.bss_ref_with_spread(est, ref, filter_length=T)
    return _cases[S, T, L]


@pytest.mark.parametrize("S,T,L", SHAPES + [(3, 512, 8000)])
def test_bss_eval_meets_the_gate(S, T, L):
    from fqss_amd import kernels as K
    est, ref, want, U = case(S, T, L)
    got = K.bss_eval(torch.from_numpy(est).cuda(), torch.from_numpy(ref).cuda(), filter_length=T).cpu().numpy()
    H.check(got, want, U, f"S = {S}, T = {T}, L = {L}")
    if S == 1:
        assert np.all(np.isposinf(got[1]))


@pytest.mark.parametrize("S,T,L", [(2, PANEL + 8, 1000), (3, PANEL // 3 + 1, 2500)])
def test_sdr_row_permutation_pitched_rows_and_repeatability(S, T, L):
    from fqss_amd import kernels as K
    est, ref, want, U = case(S, T, L)
    e, r = torch.from_numpy(est).cuda(), torch.from_numpy(ref).cuda()
    got = K.bss_eval(e, r, filter_length=T)
    # the SDR row is kernels.sdr of the matched pairs
    H.check(got[0].cpu().numpy(), K.sdr(e, r, filter_length=T).cpu().numpy(), U[0], "SDR row against kernels.sdr")
    # a non-identity permutation: estimate j against target tgt[j]
    tgt = [(j + 1) % S for j in range(S)]
    pw, pU = H.bss_ref_with_spread(est, ref, filter_length=T, tgt=tgt)
    H.check(K.bss_eval(e, r, tgt=tgt, filter_length=T).cpu().numpy(), pw, pU, f"tgt = {tgt}")
    # zero_mean and load_diag
    ow, oU = H.bss_ref_with_spread(est + np.float32(0.05), ref - np.float32(0.03), filter_length=T, zero_mean=True, load_diag=1e-3)
    H.check(K.bss_eval(e + 0.05, r - 0.03, filter_length=T, zero_mean=True, load_diag=1e-3).cpu().numpy(), ow, oU, "zero_mean, load_diag")
    # pitched rows and a second call: the same bits
    pe, pr = torch.full((S, L + 24), 7.0, device="cuda"), torch.full((S, L + 40), -3.0, device="cuda")
    pe[:, :L], pr[:, :L] = e, r
    assert torch.equal(K.bss_eval(pe[:, :L], pr[:, :L], filter_length=T), got), "pitched views"
    assert torch.equal(K.bss_eval(e, r, filter_length=T), got), "two calls"


def test_silent_target_and_refusals():
    from fqss_amd import _lib
    from fqss_amd import kernels as K
    est, ref, _, _ = case(2, 4, 500)
    e, r = torch.from_numpy(est).cuda(), torch.from_numpy(ref).cuda()
    silent = r.clone()
    silent[1] = 0.0
    assert torch.isnan(K.bss_eval(e, silent, filter_length=4)).all()
    with pytest.raises(_lib.FqssError, match="fqss_bss_eval"):
        K.bss_eval(e.repeat(2, 1), r.repeat(2, 1), filter_length=4)                  # S = 4
    with pytest.raises(_lib.FqssError, match="fqss_bss_eval"):
        K.bss_eval(e, r, filter_length=513)
    need = _lib.query("fqss_bss_eval_ws_doubles", 2, 500, 4)
    ws, out = torch.empty(need, device="cuda", dtype=torch.float64), torch.empty(3, 2, device="cuda", dtype=torch.float64)
    args = (e.data_ptr(), r.data_ptr(), None, ws.data_ptr())
    tail = (out.data_ptr(), 2, 500, 500, 500, 4, 0, -1.0, None)
    assert _lib._bind("fqss_bss_eval")(*args, need - 1, *tail) == _lib.CONSTANTS["FQSS_EINVAL"]
    assert _lib._bind("fqss_bss_eval")(*args, need, *tail) == 0
    assert need > 0 and _lib.query("fqss_bss_eval_ws_doubles", 4, 500, 4) == 0 and _lib.query("fqss_bss_eval_ws_doubles", 2, 500, 513) == 0


class Stub(torch.nn.Module):
    """[B, 1, T] -> [B, 2, T]: a two-tap low band and the rest (the generated speakers are band-split noise), element by element"""
    n_srcs, n_splitter = 2, 1

    def forward(self, x):
        lo = 0.5 * (x + torch.roll(x, 1, dims=-1))
        return torch.cat([lo, x - lo], dim=1)


def test_process_bss_eval_and_the_val_line(tmp_path, monkeypatch, capsys):
    """process.bss_eval pairs every estimate with the target of its best SI-SNR and returns the means; val.py's librimix lines are
    unchanged without `bss_eval: true` and end in ,SIR=..,SAR=.. of process.bss_eval's means with it (a two-utterance generated folder)"""
    from fqss_amd import process
    from fqss_amd import val as V
    from fqss_amd.train_env.asteroid_librimix.librimix_dataset import read_wav
    from tests.helpers_librimix import make_librimix_tree
    est, ref, _, _ = case(2, PANEL // 2, 1000)
    want, U = H.bss_ref_with_spread(est[::-1], ref, filter_length=16, tgt=[1, 0])
    got = process.bss_eval(torch.from_numpy(est[::-1].copy()).cuda(), torch.from_numpy(ref).cuda(), filter_length=16)
    H.check(got.cpu().numpy(), want.mean(axis=1), U.max(axis=1), "process.bss_eval")
    test_dir = make_librimix_tree(tmp_path, n_train=1, n_dev=2, seconds=(0.6, 0.8))["test_dir"]
    means = []
    for name in sorted(os.listdir(os.path.join(test_dir, "mix_clean"))):
        mix, s1, s2 = (torch.from_numpy(read_wav(os.path.join(test_dir, d, name))).cuda() for d in ("mix_clean", "s1", "s2"))
        clean = torch.stack([s1, s2])
        sep = process.model_infer(Stub(), mix[None], n_srcs=2, segment=8000, overlap=0.25, device="cuda", target=clean)
        means.append(process.bss_eval(sep, clean))
    sir, sar = (torch.stack(means).mean(dim=0)[1:]).tolist()
    monkeypatch.setattr(V, "create_pretrained_model", lambda model_cfg: Stub())
    lines = {}
    for flag in (False, True):
        cfg = dict(model_cfg=dict(name="stub", n_src=2, quantization=dict(qat=True)),
                   dataset_cfg=dict(name="librimix", noisy=False, sample_rate=16000, resample=1),
                   testing_cfg=dict(test_dir=test_dir, segment_samples=8000, overlap=0.25, **({"bss_eval": True} if flag else {})))
        (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
        capsys.readouterr()
        V.val(["-y", str(tmp_path / "cfg.yaml")])
        lines[flag] = capsys.readouterr().out.strip().splitlines()[-2:]
    progress, result = lines[False]
    assert progress.startswith("SI-SDR=") and "SIR" not in progress and result.startswith("SI-SDR=") and result.count(",") == 3, lines
    assert lines[True] == [progress + ",SIR={:0.3f},SAR={:0.3f}".format(sir, sar), result + ",SIR={:0.2f},SAR={:0.2f}".format(sir, sar)], lines
