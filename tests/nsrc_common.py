"""Bodies shared by tests/test_nsrc_cpu.py (CPU backend) and tests/test_gpu_nsrc.py (HIP kernels): the 1- and 3-source PIT / KD loss
against tests/golden/nsrc_loss.npz and the live oracle (oracle/fqss_oracle.py, run in float64 on the float32 inputs).

`dev(t)` places a host tensor where the selected backend wants it.  Tolerances are the project's for these kernels:
loss / kd / task rtol 1e-5, w rtol 2e-5, SI-SDR 1e-3 dB, dL/d est rtol 5e-4 with atol 2e-5 * max|g|."""
import itertools

import numpy as np
import torch

from oracle import fqss_oracle as O

PERMS = list(itertools.permutations(range(3)))


def batch3(B, T):
    """tools/make_goldens_nsrc.py's batch: sample b is built with permutation b % 6 (student) and (5b + 2) % 6 (teacher), so all six
    are selected and the 3-cycle samples select the inverse 3-cycle.  -> tgt, est, fest [B, 3, T]"""
    s = 0.05 * torch.randn(B, 3, T, generator=torch.Generator().manual_seed(1))
    e, f = torch.empty_like(s), torch.empty_like(s)
    for b in range(B):
        e[b] = s[b, list(PERMS[b % 6])] + 0.3 * 0.05 * torch.randn(3, T, generator=torch.Generator().manual_seed(10 + b))
        f[b] = s[b, list(PERMS[(5 * b + 2) % 6])] + 0.2 * 0.05 * torch.randn(3, T, generator=torch.Generator().manual_seed(20 + b))
    return s, e, f


def batch1(B, T):
    """one source (enh_single): sample b's estimate carries (1 + b % 3) * 0.1 of noise, so the weights differ"""
    s = 0.05 * torch.randn(B, 1, T, generator=torch.Generator().manual_seed(2))
    n = 0.05 * torch.randn(B, 1, T, generator=torch.Generator().manual_seed(3))
    m = 0.05 * torch.randn(B, 1, T, generator=torch.Generator().manual_seed(4))
    scale = (1.0 + torch.arange(B) % 3).view(B, 1, 1) * 0.1
    return s, s + scale * n, s + 0.2 * m


def batch(S, B, T):
    return batch3(B, T) if S == 3 else batch1(B, T)


def close_grad(got, want, msg=""):
    want = np.asarray(want)
    np.testing.assert_allclose(got, want, rtol=5e-4, atol=2e-5 * float(np.abs(want).max()), err_msg=msg)


def check_fixture(K, dev, g):
    """the reference-generated three-source objective: every figure of the fixture"""
    est, fest, tgt = (dev(torch.from_numpy(g[k])) for k in ("est", "fest", "tgt"))
    out, w, sisdr, gest = K.kd_loss(est, fest, tgt, 0.1)
    np.testing.assert_allclose(out[0].item(), g["loss"], rtol=1e-5)
    np.testing.assert_allclose(out[3].item(), g["kd"], rtol=1e-5)
    np.testing.assert_allclose(out[2].item(), g["task"], rtol=1e-5)
    np.testing.assert_allclose(out[1].item(), -10 * np.log10(g["kd"] + 1e-8), rtol=1e-5)
    np.testing.assert_allclose(w.cpu().numpy(), g["w"], rtol=2e-5)
    np.testing.assert_allclose(sisdr.cpu().numpy(), -g["sdrqs"], atol=1e-3)
    got = gest.cpu().numpy()
    for b in range(got.shape[0]):       # per sample, so that a wrong pairing in one of them names it (3 and 4 are the 3-cycles)
        close_grad(got[b], g["gest"][b], f"sample {b}")
    # the teacher-free form on the same estimate: its per-sample SI-SDR is the fixture's sdrqs
    out2, sisdr2, _ = K.pit_sisdr_loss(est, tgt)
    np.testing.assert_allclose(out2[0].item(), float(np.mean(g["sdrqs"])), rtol=1e-5)
    np.testing.assert_allclose(sisdr2.cpu().numpy(), -g["sdrqs"], atol=1e-3)


def check_kd_loss(K, dev, S, B, T):
    """mode 0 against O.kd_loss"""
    s, e, f = batch(S, B, T)
    er = e.double().requires_grad_(True)
    loss, kd, task, w_r, sdrs, sdrqs = O.kd_loss(er, f.double(), s.double())
    loss.backward()
    out, w, sisdr, gest = K.kd_loss(dev(e), dev(f), dev(s), 0.1)
    msg = f"S={S} B={B} T={T}"
    np.testing.assert_allclose(out[0].item(), loss.item(), rtol=1e-5, err_msg=msg)
    np.testing.assert_allclose(out[3].item(), kd.item(), rtol=1e-5, err_msg=msg)
    np.testing.assert_allclose(out[2].item(), task.item(), rtol=1e-5, err_msg=msg)
    np.testing.assert_allclose(w.cpu().numpy(), w_r.numpy(), rtol=2e-5, err_msg=msg)
    np.testing.assert_allclose(sisdr.cpu().numpy(), -sdrqs.numpy(), atol=1e-3, err_msg=msg)
    close_grad(gest.cpu().numpy(), er.grad.numpy(), msg)
    assert K.kd_loss(dev(e), dev(f), dev(s), 0.1, want_grad=False)[3] is None


def check_pit_sisdr(K, dev, S, B, T):
    """mode 2 against O.neg_sisdr_pit"""
    s, e, _ = batch(S, B, T)
    er = e.double().requires_grad_(True)
    loss = O.neg_sisdr_pit(er, s.double())
    loss.backward()
    per = torch.stack([O.neg_sisdr_pit(e[b:b + 1].double(), s[b:b + 1].double()) for b in range(B)])
    out, sisdr, gest = K.pit_sisdr_loss(dev(e), dev(s))
    msg = f"S={S} B={B} T={T}"
    np.testing.assert_allclose(out[0].item(), loss.item(), rtol=1e-5, err_msg=msg)
    np.testing.assert_allclose(sisdr.cpu().numpy(), -per.numpy(), atol=1e-3, err_msg=msg)
    close_grad(gest.cpu().numpy(), er.grad.numpy(), msg)


def check_speechbrain(K, dev, S, T, first=0):
    """mode 1 against O.kd_loss_speechbrain at B = 1 and B = S: no threshold, -30, 1e9, and at B > 1 one threshold between the
    oracle's smallest and largest per-sample loss.  `first`: where the B samples start in the batch (3: the two 3-cycles are in)"""
    s_all, e_all, f_all = batch(S, first + S, T)
    for B in sorted({1, S}):
        e, f, t = e_all[first:first + B], f_all[first:first + B], s_all[first:first + B]
        _, per, _ = O.kd_loss_speechbrain(e.double(), f.double(), t.double())
        ths = [None, -30.0, 1e9] + ([0.5 * (per.min() + per.max()).item()] if B > 1 else [])
        for th in ths:
            er = e.double().requires_grad_(True)
            loss, per_r, w_r = O.kd_loss_speechbrain(er, f.double(), t.double(), threshold=th)
            loss.backward()
            out, w, sisdr, gest = K.kd_loss(dev(e), dev(f), dev(t), 0.1, per_sample=True, threshold=th)
            msg = f"S={S} B={B} T={T} th={th}"
            np.testing.assert_allclose(out[0].item(), loss.item(), rtol=1e-5, err_msg=msg)
            np.testing.assert_allclose(w.cpu().numpy(), w_r.numpy(), rtol=2e-5, err_msg=msg)
            close_grad(gest.cpu().numpy(), er.grad.numpy(), msg)
        if B > 1:
            assert per.min().item() < ths[-1] < per.max().item()


def check_moments(K, dev, S, B, T):
    """fqss_kd_moments_n against float64 sums: each moment within 1e-11 * sum |a||b| (fp64 accumulation of at most 2e4 exactly
    representable products; the order of the additions is all that differs)"""
    s, e, f = batch(S, B, T)
    m = K.kd_moments(dev(e), dev(f), dev(s)).cpu()
    sig = torch.cat([e, f, s], dim=1).double()                     # e_0.. f_0.. t_0..
    one = torch.ones(B, 1, T, dtype=torch.float64)
    def pair(a, b):                                                # -> value, bound: [B, na, nb]
        return torch.einsum("bit,bjt->bij", a, b), 1e-11 * torch.einsum("bit,bjt->bij", a.abs(), b.abs())
    E, Fq, Tg = sig[:, :S], sig[:, S:2 * S], sig[:, 2 * S:]
    v, bd = pair(sig, one)
    want, bound = [v.reshape(B, -1), (sig * sig).sum(-1)], [bd.reshape(B, -1), 1e-11 * (sig * sig).sum(-1)]
    for a, b in ((E, Tg), (E, Fq), (Fq, Tg)):
        v, bd = pair(a, b)
        want.append(v.reshape(B, -1)), bound.append(bd.reshape(B, -1))
    want, bound = torch.cat(want, dim=1), torch.cat(bound, dim=1)
    n = 6 * S + 3 * S * S
    assert want.shape == (B, n) and m.shape == (B, K.KD_STATS_STRIDE_N)
    err = (m[:, :n] - want).abs()
    assert bool((err <= bound).all()), (f"S={S} B={B} T={T}", float((err / bound).max()))
    assert float(m[:, n:].abs().max()) == 0.0                      # the rest of the row is zeroed, not left as it was


TINY = dict(n_spks=3, kernel_size=16, stride=8, n_filters=32, bn_chan=16, hid_chan=32, n_blocks=2, n_repeats=1)


def tiny_pair(device, seed=0, **kw):
    from fqss_amd import smoke
    return smoke.build_pair(device, seed, **dict(TINY, **kw))


def check_tiny_training(device, n_steps=2):
    """steps 1-2 of KDTrainStep on a tiny three-source ConvTasNetQ against the oracle's Trainer on the same initial state, with the
    step-1/2 tolerances of tests/test_gpu_model.py::test_tiny_training_vs_reference_goldens"""
    from fqss_amd import data
    from fqss_amd.runtime import KDTrainStep
    model, fmodel = tiny_pair(device)
    sd0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    fsd = {k: v.detach().cpu().clone() for k, v in fmodel.state_dict().items()}
    x, tgt = data.synth_batch(2, 800, seed=0, n_src=3)
    assert tgt.shape == (2, 3, 800)
    student = O.StudentConvTasNetQ(sd0, n_src=3, layers_per_stack=2)
    ref = O.Trainer(student, O.TeacherConvTasNet(fsd, n_src=3, layers_per_stack=2))
    step = KDTrainStep(model, fmodel, kd_lambda=0.1, lr=1e-3, clip=5.0)
    for s in range(1, n_steps + 1):
        r = step(x.to(device), tgt.to(device))
        want = ref.step(x, tgt)
        p = f"step {s}"
        assert r["est"].shape == (2, 3, 800)
        np.testing.assert_allclose(r["loss"].item(), want["loss"].item(), rtol=1e-5, err_msg=p)
        np.testing.assert_allclose(r["kd"].item(), want["kd"].item(), rtol=1e-5, err_msg=p)
        np.testing.assert_allclose(r["w"].cpu().numpy(), want["w"].numpy(), rtol=2.3e-4, err_msg=p)
        np.testing.assert_allclose(r["sisdr"].cpu().numpy(), -want["sdrqs"].numpy(), atol=1e-3, err_msg=p)
        np.testing.assert_allclose(r["est"].cpu().numpy(), want["est"].detach().numpy(), rtol=1e-4, atol=2e-6, err_msg=p)
        np.testing.assert_allclose(r["gnorm"].item(), float(want["gnorm"]), rtol=1e-4, err_msg=p)
        coef = min(1.0, 5.0 / (float(want["gnorm"]) + 1e-6))       # the oracle's gradients are clipped in place
        n_checked = 0
        for name, prm in model.named_parameters():
            gr = student.p[name].grad
            if gr is None:
                assert float(prm.grad.abs().max()) == 0.0, name
                continue
            gr = gr.numpy() / coef
            if float(np.abs(gr).max()) == 0.0:
                continue
            err = np.linalg.norm(prm.grad.cpu().numpy() - gr) / np.linalg.norm(gr)
            assert err <= 2e-3, (p, name, err)
            n_checked += 1
        assert n_checked >= 30
    return model, step
