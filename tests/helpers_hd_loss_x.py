"""fqss_hd_loss_x restated in float64 (include/fqss.h), and the cases, gates and case body its GPU and CPU tests share.

Gates, relative to a field's largest value.  Without a teacher every field of `out` is an fp64 value rounded once to fp32 (2^-24):
2 x 2^-24; kd_s is exactly 0, w exactly 1; the gradient is one fp32 coefficient times an exact sign or one fp32 difference: 4 x 2^-24.
With a teacher w goes through the statement's fp32 log10f / expf sequence, and kd_s, loss (all of it where the task term vanishes, as
at N = 1 here) and the gradient inherit it: the bounds tests/test_gpu_norm_kernels.py records for the l1 + teacher case, w 3e-6 and kd 1.4e-6,
and 1.8e-6 for the gradient.  Measured on an MI355X, largest over the cases: without a teacher 4.1e-8 (fields), 7.6e-8 (mse gradient),
3.0e-8 (l1 gradient); with one w 9.7e-7, kd_s 5.6e-7, loss 5.3e-7, gradient 5.1e-7, reco / nsdr 3.9e-8 -- the gates are 2.5 .. 3.5 x.
The CPU backend (fp64 sums in index order): 5.0e-7, 5.6e-7, 5.3e-7, 5.1e-7."""
import numpy as np
import torch

TILE = 4096
# (B, S, N): one sample, below one vector, one short of / one over a tile, several tiles with odd N (rows after the first misaligned)
SHAPES = [(1, 1, 1), (1, 1, 3), (2, 2, TILE - 1), (1, 1, TILE + 1), (4, 4, 2 * TILE + 1027)]
MODES = [("l1", True), ("l1", False), ("mse", False)]       # (kind, teacher)
FIELDS = ("loss", "reco", "nsdr", "loss_s", "reco_s", "nsdr_s", "kd_s", "w")
ULPS = 2 * 2.0 ** -24
GATE = {True: dict(loss=1.4e-6, reco=ULPS, nsdr=ULPS, loss_s=1.4e-6, reco_s=ULPS, nsdr_s=ULPS, kd_s=1.4e-6, w=3e-6, gest=1.8e-6),
        False: dict(loss=ULPS, reco=ULPS, nsdr=ULPS, loss_s=ULPS, reco_s=ULPS, nsdr_s=ULPS, kd_s=0.0, w=0.0, gest=2 * ULPS)}


def case(B, S, N, teacher=True, device="cpu"):
    # unequal weights; source S-1 of item 0 silent (P = 0), est == src on the last item (Q = 0), exact ties elsewhere (sign(0) = 0)
    g = torch.Generator().manual_seed(7 * N + B)
    src = torch.randn(B, S, N, generator=g) * 0.1
    est = src + torch.randn(B, S, N, generator=g) * 0.03
    fest = src + torch.randn(B, S, N, generator=g) * 0.02
    est[..., ::5] = src[..., ::5]
    est[..., 1::7] = fest[..., 1::7]
    if B * S > 1:
        src[0, S - 1] = 0.0
        est[B - 1, S - 1] = src[B - 1, S - 1]
    wt = torch.arange(1, S + 1, dtype=torch.float32) / 2
    est, fest, src, wt = (t.to(device) for t in (est, fest, src, wt))
    return (est, fest, src, wt, 0.1) if teacher else (est, None, src, wt, 0.0)


def ref(est, fest, src, wt, lam, kind):      # every field of `out` and dloss/dest in float64
    e, s, w8 = est.double().cpu().numpy(), src.double().cpu().numpy(), wt.double().cpu().numpy()
    B, S, N = e.shape
    lam = float(np.float32(lam))        # the C ABI takes kd_lambda as a float
    A, Q, P = np.abs(e - s).sum(-1), ((e - s) ** 2).sum(-1), (s ** 2).sum(-1)
    nsdr_bs = 10 * np.log10((P + 1e-7) / (Q + 1e-7))
    c = w8 / w8.sum() / (B * N)
    w, kd_s = np.ones((B, S)), np.zeros(S)
    if kind == "mse":
        loss_s, reco_s, g = (Q / N).mean(0), np.sqrt(Q / N).mean(0), 2 * c[None, :, None] * (e - s)
    else:
        loss_s = reco_s = (A / N).mean(0)
        g = c[None, :, None] * np.sign(e - s)
        if fest is not None:
            f = fest.double().cpu().numpy()
            w = np.exp((10 * np.log10((P + 1e-7) / (((s - f) ** 2).sum(-1) + 1e-7)) - nsdr_bs) / 10)
            kd_s = (w * np.abs(e - f).sum(-1) / N).mean(0)
            loss_s = (1 - lam) * reco_s + lam * kd_s
            g = (1 - lam) * g + lam * (c[None] * w)[..., None] * np.sign(e - f)
    mean = lambda v: (w8 * v).sum() / w8.sum()
    return dict(loss=mean(loss_s), reco=mean(reco_s), nsdr=mean(nsdr_bs.mean(0)), loss_s=loss_s, reco_s=reco_s, nsdr_s=nsdr_bs.mean(0),
                kd_s=kd_s, w=w, gest=g)


def rel_err(got, want):      # largest |got - want| over the largest |want| of the field
    got, want = np.asarray(got.cpu() if torch.is_tensor(got) else got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def check_case(kind, teacher, shape, want_grad, device):
    from fqss_amd import kernels as K
    ops = case(*shape, teacher=teacher, device=device)
    want = ref(*ops, kind)
    got = K.hd_loss_x(*ops, kind=kind, want_grad=want_grad)
    assert (got.gest is not None) == want_grad
    for n in FIELDS + (("gest",) if want_grad else ()):
        assert rel_err(getattr(got, n), want[n]) <= GATE[teacher][n], (n, rel_err(getattr(got, n), want[n]))
    if want_grad:
        assert (got.gest.cpu().numpy()[want["gest"] == 0] == 0).all(), "sign(0) = 0: a tie gives an exactly zero gradient"


def check_refusals(device):      # mse takes no teacher; a distillation weight needs one
    from fqss_amd import _lib, kernels as K
    import pytest
    est, fest, src, wt, _ = case(2, 2, 64, device=device)
    for f, lam, kind in ((fest, 0.0, "mse"), (None, 0.1, "l1")):
        with pytest.raises(_lib.FqssError, match="fqss_hd_loss_x"):
            K.hd_loss_x(est, f, src, wt, lam, kind=kind)
