"""Bodies of the optimizer-family kernel tests (fqss.h: fqss_optim_clip, fqss_ema_update, fqss_ema_update_dev), run by
tests/test_optim_cpu.py on the CPU backend and by tests/test_gpu_optim.py on the HIP kernels.  Every reference is torch.optim itself
(or fp64 arithmetic) on the CPU, computed once per case and shared."""
import functools

import numpy as np
import pytest
import torch

from fqss_amd import _lib
from fqss_amd import kernels as K

RTOL, ATOL = 1e-6, 1e-7         # the project's bound for this kernel (tests/test_gpu_kernels.py test_adam_clip_vs_torch)
SIZES = (100003, 1, 63, 64, 65, 257)
STEPS = 5
NEVER = 2 ** 31 - 1
# (kind, lr, decay, momentum, nesterov).  Adam with L2 decay is ill-conditioned where g + wd * p cancels: tests/test_optim_cpu.py's
# docstring says how its decay and the scaled steps of grads() were chosen
CASES = {"adam_l2": ("adam", 1e-3, 1e-3, 0.0, False), "adamw_1e-2": ("adamw", 1e-3, 1e-2, 0.0, False),
         "adamw_0.1": ("adamw", 1e-3, 0.1, 0.0, False), "sgd_momentum": ("sgd", 1e-2, 1e-2, 0.9, False),
         "sgd_nesterov": ("sgd", 1e-2, 1e-2, 0.9, True)}


def device():
    return "cpu" if _lib.BACKEND == "cpu" else "cuda"


def rnd(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


def grads(n):
    """the data of test_adam_clip_vs_torch (g ~ 0.05 N(0, 1)), every second step -- the first, third and fifth -- scaled by 3.0 so
    that the clip engages (see tests/test_optim_cpu.py's docstring for why not the second and fourth)"""
    g = rnd(n, 2, 0.05)
    return [g * (1.0 if it % 2 else 3.0) for it in range(STEPS)]


def torch_optimizer(groups, kind, lr, wd, mu, nesterov):
    if kind == "adam":
        return torch.optim.Adam(groups, lr=lr, weight_decay=wd, foreach=False)
    if kind == "adamw":
        return torch.optim.AdamW(groups, lr=lr, weight_decay=wd, foreach=False)
    return torch.optim.SGD(groups, lr=lr, weight_decay=wd, momentum=mu, nesterov=nesterov, foreach=False)


def torch_moments(opt, p, kind):
    st = opt.state[p]
    if kind == "sgd":
        return st["momentum_buffer"], None
    return st["exp_avg"], st["exp_avg_sq"]


class Flat:
    """the buffers of one fqss_optim_clip run where the selected backend computes"""

    def __init__(self, p0, t0=None, shift=0):
        d, n = device(), p0.numel()
        # shift = 1: every buffer starts one float past a 16-B boundary (the scalar-access form of the HIP kernel)
        mk = lambda src: torch.cat([torch.zeros(shift), src]).to(d)[shift:]
        self.p, self.m, self.v = mk(p0), mk(torch.zeros(n)), mk(torch.zeros(n))
        self.t0 = None if t0 is None else torch.cat([torch.zeros(shift, dtype=torch.int32), t0]).to(d)[shift:]
        self.acc = torch.zeros(1, device=d, dtype=torch.float64)
        self.step = torch.zeros(1, device=d, dtype=torch.int32)
        self.gn = torch.zeros(1, device=d)
        self.shift = shift

    def g(self, g):
        return torch.cat([torch.zeros(self.shift), g]).to(device())[self.shift:]

    def update(self, g, lr, fused="optim", **kw):
        g = self.g(g)
        self.acc.zero_()
        K.sumsq(g, self.acc)
        if fused == "adam":
            K.adam_clip(self.p, g, self.m, self.v, self.acc, self.step, self.gn, 5.0, 1.0, lr, t0=self.t0)
        else:
            K.optim_clip(self.p, g, self.m, self.v, self.acc, self.step, self.gn, 5.0, 1.0, lr, t0=self.t0, **kw)


@functools.lru_cache(maxsize=None)
def reference(case, n):
    """torch.optim on the CPU: the parameters and the gradient norm after each of the 5 steps, the moments after the last"""
    kind, lr, wd, mu, nesterov = CASES[case]
    p = rnd(n, 1).requires_grad_(True)
    opt = torch_optimizer([p], kind, lr, wd, mu, nesterov)
    ps, norms = [], []
    for g in grads(n):
        p.grad = g.clone()
        norms.append(float(torch.nn.utils.clip_grad_norm_([p], 5.0)))
        opt.step()
        ps.append(p.detach().clone())
    m, v = torch_moments(opt, p, kind)
    return ps, norms, m.clone(), None if v is None else v.clone()


def close(got, want, what):
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=RTOL, atol=ATOL, err_msg=what)


def check_vs_torch(case, n, shift=0):
    kind, lr, wd, mu, nesterov = CASES[case]
    ps, norms, m, v = reference(case, n)
    f = Flat(rnd(n, 1), shift=shift)
    for it, g in enumerate(grads(n)):
        f.update(g, lr, kind=kind, weight_decay=wd, momentum=mu, nesterov=nesterov)
        np.testing.assert_allclose(f.gn.item(), norms[it], rtol=1e-6)
        close(f.p, ps[it], f"{case} n={n} step {it + 1}: p")
    close(f.m, m, f"{case} n={n}: first moment / momentum buffer")
    if v is not None:
        close(f.v, v, f"{case} n={n}: second moment")
    assert f.step.item() == STEPS


def check_adam_bits(n, shift=0):
    """kind = adam, no decay, no table: the bits of fqss_adam_clip"""
    a, b = Flat(rnd(n, 1), shift=shift), Flat(rnd(n, 1), shift=shift)
    for g in grads(n):
        a.update(g, 1e-3, fused="adam")
        b.update(g, 1e-3, kind="adam", weight_decay=0.0)
        for x, y, what in ((a.p, b.p, "p"), (a.m, b.m, "m"), (a.v, b.v, "v"), (a.gn, b.gn, "gnorm"), (a.step, b.step, "step_t")):
            assert torch.equal(x, y), (n, what)


def check_clocks(case):
    """elements 0::3 are live from the first step, 1::3 first see a gradient at step 3 (t0 = 2), 2::3 never do (t0 = INT32_MAX)"""
    kind, lr, wd, mu, nesterov = CASES[case]
    k = 1371
    n = 3 * k
    p0, gs = rnd(n, 1), grads(n)
    t0 = torch.tensor([0, 2, NEVER], dtype=torch.int32).repeat(k)
    pa, pb = p0[0::3].clone().requires_grad_(True), p0[1::3].clone().requires_grad_(True)
    opt = torch_optimizer([pa, pb], kind, lr, wd, mu, nesterov)
    f = Flat(p0, t0=t0)
    f.m.copy_(rnd(n, 5) * (t0 == NEVER))      # what the never-used third holds must survive bit for bit
    f.v.copy_(rnd(n, 6).abs() * (t0 == NEVER))
    m0, v0 = f.m.clone(), f.v.clone()
    for it, g in enumerate(gs):
        g = g.clone()
        g[2::3] = 0.0                          # a parameter without a gradient: zeros in the arena
        pa.grad = g[0::3].clone()
        if it >= 2:
            pb.grad = g[1::3].clone()
        else:
            g[1::3] = 0.0
        live = [pa, pb] if it >= 2 else [pa]
        norm = float(torch.nn.utils.clip_grad_norm_(live, 5.0))
        opt.step()
        f.update(g, lr, kind=kind, weight_decay=wd, momentum=mu, nesterov=nesterov)
        np.testing.assert_allclose(f.gn.item(), norm, rtol=1e-6)
        close(f.p[0::3], pa.detach(), f"{case} step {it + 1}: live from the start")
        close(f.p[1::3], pb.detach(), f"{case} step {it + 1}: live from step 3")
        if it < 2:
            for buf, was in ((f.p, p0), (f.m, m0.cpu()), (f.v, v0.cpu())):
                assert torch.equal(buf[1::3].cpu(), was[1::3])
    for buf, was in ((f.p, p0), (f.m, m0.cpu()), (f.v, v0.cpu())):
        assert torch.equal(buf[2::3].cpu(), was[2::3]), "an element without a gradient was touched"
    mb, vb = torch_moments(opt, pb, kind)
    close(f.m[1::3], mb, f"{case}: moment of the late parameter (SGD: cloned from its first gradient)")
    if vb is not None:
        close(f.v[1::3], vb, f"{case}: second moment of the late parameter")


def check_slot_table(case):
    """three 64-float slots with decays (0, 1e-2, 0.1) = three torch parameter groups"""
    kind, lr, _, mu, nesterov = CASES[case]
    decays, n = (0.0, 1e-2, 0.1), 192
    p0 = rnd(n, 1)
    ps = [p0[64 * i:64 * i + 64].clone().requires_grad_(True) for i in range(3)]
    opt = torch_optimizer([{"params": [p], "weight_decay": wd} for p, wd in zip(ps, decays)], kind, lr, 0.5, mu, nesterov)
    f = Flat(p0)
    table = torch.tensor(decays, dtype=torch.float32, device=device())
    for it, g in enumerate(grads(n)):
        for i, p in enumerate(ps):
            p.grad = g[64 * i:64 * i + 64].clone()
        torch.nn.utils.clip_grad_norm_(ps, 5.0)
        opt.step()
        f.update(g, lr, kind=kind, weight_decay=0.5, wd_slot=table, momentum=mu, nesterov=nesterov)   # (the table overrides the scalar)
        close(f.p, torch.cat([p.detach() for p in ps]), f"{case} step {it + 1}: p under the slot table")


def check_ema(n, on_device, shift=0):
    """U = 5 updates of the unbiased form at decay 0.999 against fp64.  Bound U * 3 * 2^-24 * max|operand|: per update the two products
    and the sum round once each; the rounded scalars w and 1 - w scale operands that sum to at most max|operand| * (w + 1 - w)."""
    U, decay, d = 5, 0.999, device()
    mk = lambda src: torch.cat([torch.zeros(shift), src]).to(d)[shift:]
    ema = mk(rnd(n, 3))
    ref = rnd(n, 3).double()
    count_dev = torch.zeros(1, dtype=torch.float64, device=d)
    count, top = 0.0, float(ref.abs().max())
    for u in range(U):
        p = rnd(n, 10 + u)
        count = count * decay + 1.0
        if on_device:
            w = 1.0 / count
            K.ema_update(ema, mk(p), decay=decay, count=count_dev)
            assert count_dev.item() == count
        else:
            w = float(np.float32(1.0 / count))        # the operand the entry point is given
            K.ema_update(ema, mk(p), w=w)
        ref = ref * (1.0 - w) + w * p.double()
        top = max(top, float(p.abs().max()), float(ref.abs().max()))
    err = float((ema.cpu().double() - ref).abs().max())
    bound = U * 3 * 2.0 ** -24 * top
    print(f"ema_update n={n} device_count={on_device}: max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)


# ---- refusals: non-zero return, nothing launched, every buffer as it was ------------------------------------------------------------
def _optim_args(f, grad, **over):
    a = dict(p=f.p, g=grad, m=f.m, v=f.v, n=f.p.numel(), sumsq=f.acc, max_norm=5.0, grad_scale=1.0, lr=1e-3, beta1=0.9, beta2=0.999,
             eps=1e-8, step_t=f.step, t0=None, gnorm_out=f.gn, kind=0, weight_decay=0.0, wd_slot=None, momentum=0.0, nesterov=0)
    a.update(over)
    ptr = lambda t: None if t is None else t.data_ptr()
    return [ptr(a[k]) if k in ("p", "g", "m", "v", "sumsq", "step_t", "t0", "gnorm_out", "wd_slot") else a[k] for k in a] + [K._stream()]


REFUSED = {"unknown kind": dict(kind=3), "negative kind": dict(kind=-1), "negative decay": dict(weight_decay=-1e-3),
           "momentum 1": dict(kind=2, momentum=1.0), "negative momentum": dict(kind=2, momentum=-0.1),
           "nesterov without momentum": dict(kind=2, nesterov=1), "null p": dict(p=None), "null g": dict(g=None),
           "table with n % 64 != 0": dict(wd_slot="table", n=100)}


def check_refusal(name):
    f = Flat(rnd(128, 1))
    f.m.copy_(rnd(128, 2))
    f.v.copy_(rnd(128, 3).abs())
    g = rnd(128, 4).to(device())
    f.acc.fill_(4.0)
    over = dict(REFUSED[name])
    if over.get("wd_slot") == "table":
        over["wd_slot"] = torch.full((2,), 0.01, device=device())
    before = [t.clone() for t in (f.p, f.m, f.v, f.step, f.gn, g)]
    rc = _lib._bind("fqss_optim_clip")(*_optim_args(f, g, **over))
    if device() == "cuda":
        torch.cuda.synchronize()
    assert rc != 0, name
    assert _lib.load().fqss_last_error()
    for was, now in zip(before, (f.p, f.m, f.v, f.step, f.gn, g)):
        assert torch.equal(was, now), name
    assert _optim_args(f, g)[15] == 0 and _lib._bind("fqss_optim_clip")(*_optim_args(f, g)) == 0     # ... and the plain call is taken


def check_ema_refusals():
    d = device()
    buf, p = rnd(150, 1).to(d), rnd(100, 2).to(d)
    count = torch.zeros(1, dtype=torch.float64, device=d)
    was = buf.clone()
    ema, over = buf[:100], buf[50:150]
    s = K._stream()
    for name, args in (("fqss_ema_update", (ema.data_ptr(), over.data_ptr(), 100, 0.5, s)),
                       ("fqss_ema_update", (over.data_ptr(), ema.data_ptr(), 100, 0.5, s)),
                       ("fqss_ema_update", (None, p.data_ptr(), 100, 0.5, s)), ("fqss_ema_update", (ema.data_ptr(), None, 100, 0.5, s)),
                       ("fqss_ema_update_dev", (ema.data_ptr(), over.data_ptr(), 100, 0.9, count.data_ptr(), s)),
                       ("fqss_ema_update_dev", (None, p.data_ptr(), 100, 0.9, count.data_ptr(), s)),
                       ("fqss_ema_update_dev", (ema.data_ptr(), p.data_ptr(), 100, 0.9, None, s))):
        assert _lib._bind(name)(*args) != 0, (name, args)
    assert _lib._bind("fqss_ema_update")(ema.data_ptr(), p.data_ptr(), 0, 0.5, s) == 0                      # n = 0: a no-op
    assert _lib._bind("fqss_ema_update_dev")(ema.data_ptr(), p.data_ptr(), 0, 0.9, count.data_ptr(), s) == 0
    if d == "cuda":
        torch.cuda.synchronize()
    assert torch.equal(buf, was) and count.item() == 0.0
    with pytest.raises(_lib.FqssError):
        K.ema_update(ema, rnd(99, 1).to(d), w=0.5)
