"""GPU: LSTMQ_static -- the quantized recurrence kernels (csrc/lstmq.hip: fqss_lstmq_fwd / fqss_lstmq_bwd), ops_dp.LstmBiQ and the
module against the reference's recorded runs (tests/golden/lstmq_static.npz, tools/make_goldens_lstmq.py).

Gate G1 (tests/test_gpu_model.py): every bin index within 1 of the reference's, at most 2e-3 of them different.  It is a cap, not a
measurement: the generator shows that the fp32 reference stays inside it against its own fp64 run for the committed seed.
Shapes: H = 8 (4H = 32 threads, less than one wave; S = 6 is no multiple of the 4-step prefetch ring; B = 3 leaves the last
workgroup's second sequence absent), H = 24 (4H no multiple of 64: gate kinds share a wave), H = 128 (the cfg-3 width: the register-
resident forward k_lstmq_fwd_st<128>, S = 6 and a single step; the backward's 512-thread build) and H = 136 (back on the generic forward;
the backward's 1024-thread build).  The H = 128 forward is held against the generic kernel at that width (the test hook
fqss_lstmq_fwd_generic behind kernels.LSTMQ_GENERIC_FWD) on every output and saved image, and against the step-by-step path."""
import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

P = dict(gradient_based=True, weight_quant=True, act_quant=True, act_n_bits=8, weight_n_bits=8)
I_DIM = 16


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _idx_stats(y, y_ref, lo, hi):
    delta = (hi - lo) / 255.0
    a, b = np.rint((y - lo) / delta), np.rint((y_ref - lo) / delta)
    return float(np.mean(a != b)), float(np.abs(a - b).max())


def _g1(y, y_ref, lo, hi, what):
    frac, dmax = _idx_stats(np.asarray(y, dtype=np.float64), np.asarray(y_ref, dtype=np.float64), lo, hi)
    print(f"{what}: differing fraction {frac:.3e}, largest index distance {dmax:.0f}")
    assert dmax <= 1 and frac <= 2e-3, (what, frac, dmax)


def _leave_observer(L):
    from fqss_amd.quantization.qat import qat_quant as QQ
    for m in L.modules():
        if isinstance(m, QQ.GradientActivationFakeQuantize):
            m.n_iter = m.max_observations
        if isinstance(m, QQ.GradientWeightFakeQuantize):
            m.observer_mode = False


def _fixture_layer(g, case):
    from fqss_amd.quantization.qat import qat_layers as QL
    sd = {k[len(case) + 4:]: T(g[k]) for k in g.files if k.startswith(case + ".sd.")}
    H = sd["lstm.weight_hh_l0"].shape[1]
    L = QL.LSTMQ_static(nn.LSTM(I_DIM, H, 1, bidirectional=True), **P)
    L.load_state_dict(sd, strict=True)
    return L.cuda().train(), H


def _random_layer(H, seed):
    """a calibrated layer without a fixture: keyed weights, ranges from ONE observing forward of S = 56 > 50 steps (the module's own
    calibration path), then tightened so that both clip branches are taken"""
    from fqss_amd.quantization.qat import qat_layers as QL
    from fqss_amd.quantization.qat import qat_quant as QQ
    gen = torch.Generator().manual_seed(seed)
    L = QL.LSTMQ_static(nn.LSTM(I_DIM, H, 1, bidirectional=True), **P)
    with torch.no_grad():
        for k, p in L.named_parameters():
            if not k.endswith("_range"):
                p.copy_(torch.randn(p.shape, generator=gen) * (0.1 if p.dim() == 1 else 1.2 / np.sqrt(p.shape[1])))
    L = L.cuda().train()
    with torch.no_grad():
        L(torch.randn(56, 2, I_DIM, generator=gen).cuda())
        for n, m in L.named_children():
            if isinstance(m, QQ.GradientActivationFakeQuantize) and n != "activation_fake_quantize_mul2_r":
                lo, hi = m.min_range.item(), m.max_range.item()
                m.min_range.fill_((lo + hi) / 2 - 0.93 * (hi - lo) / 2)
                m.max_range.fill_((lo + hi) / 2 + 0.93 * (hi - lo) / 2)
    _leave_observer(L)
    return L, gen


def _kernel_operands(L):
    """(wih [8H, I], bih [8H], whh [2, 4H, H], bhh [2, 4H], ranges) as LstmBiQ hands them to the kernels"""
    from fqss_amd import kernels as K
    with torch.no_grad():
        w = {n: q(getattr(L.lstm, n)).detach() for n, q in L.weight_quantizers_dict.items()}
    wih = torch.cat([w["weight_ih_l0"], w["weight_ih_l0_reverse"]], 0).contiguous()
    whh = torch.stack([w["weight_hh_l0"], w["weight_hh_l0_reverse"]], 0).contiguous()
    bih = torch.cat([L.lstm.bias_ih_l0, L.lstm.bias_ih_l0_reverse], 0).detach().contiguous()
    bhh = torch.stack([L.lstm.bias_hh_l0, L.lstm.bias_hh_l0_reverse], 0).detach().contiguous()
    aqs = [getattr(L, f"activation_fake_quantize_{s}{sfx}") for sfx in ("", "_r") for s in K.LSTMQ_SITES]
    return wih, bih, whh, bhh, [(a.min_range.detach(), a.max_range.detach()) for a in aqs]


def _rng(g, case, q):
    return float(g[f"{case}.sd.{q}.min_range"][0]), float(g[f"{case}.sd.{q}.max_range"][0])


# ------------------------------------------------------------------------------------------------------- 2. teacher-forced forward
@pytest.mark.parametrize("case", ["q8", "q24"])
def test_kernel_forward_teacher_forced(golden, case):
    """every recorded reference step as its own batch row of ONE launch with S = 1: `pre` from the fixture's input through the package's
    row linear, the carried state the reference's own -> h on the mul2 grid, c on the add1 grids"""
    from fqss_amd import kernels as K
    g = golden("lstmq_static")
    L, H = _fixture_layer(g, case)
    _leave_observer(L)
    wih, bih, whh, bhh, ranges = _kernel_operands(L)
    x = T(g[f"{case}.x"]).cuda()
    S, B, _ = x.shape
    R = S * B
    rows = torch.stack([x.reshape(R, I_DIM), x.flip(0).reshape(R, I_DIM)])          # step k: time k forward, time S-1-k reverse
    pre = torch.cat([K.rowlin_fwd(rows[0], wih[:4 * H], bih[:4 * H]), K.rowlin_fwd(rows[1], wih[4 * H:], bih[4 * H:])], -1).reshape(1, R, 8 * H)
    state = lambda a: T(a).permute(1, 0, 2, 3).reshape(2, R, H).contiguous().cuda()        # [S, 2, B, H] -> [2, S*B, H]
    hout, hc, _, _ = K.lstmq_fwd(pre.contiguous(), whh, bhh, ranges, 1, R, H, h0=state(g[f"{case}.h_in"]), c0=state(g[f"{case}.c_in"]), save=False,
                                 want_last=True)
    torch.cuda.synchronize()
    assert torch.equal(hout.reshape(R, 2, H).permute(1, 0, 2), hc[0])
    h_ref, c_ref = state(g[f"{case}.h_out"]).cpu().numpy(), state(g[f"{case}.c_out"]).cpu().numpy()
    got = hc.cpu().numpy()
    _g1(got[0], h_ref, *_rng(g, case, "activation_fake_quantize_mul2"), f"{case} h")
    _g1(got[1, 0], c_ref[0], *_rng(g, case, "activation_fake_quantize_add1"), f"{case} c forward")
    _g1(got[1, 1], c_ref[1], *_rng(g, case, "activation_fake_quantize_add1_r"), f"{case} c reverse")


# ------------------------------------------------------------------------------------------------------------ 3. chaining is exact
def _chain_case(name, golden):
    if name == "q8":
        g = golden("lstmq_static")
        L, H = _fixture_layer(g, "q8")
        _leave_observer(L)
        x = T(g["q8.x"]).cuda()
    else:
        H, S, B = {"h128": (128, 6, 3), "h128s1": (128, 1, 3), "h136": (136, 3, 1)}[name]
        L, gen = _random_layer(H, 5)
        x = torch.randn(S, B, I_DIM, generator=gen).cuda()
    return L, H, x


@pytest.mark.parametrize("name", ["q8", "h128", "h128s1", "h136"])
def test_kernel_chaining_is_exact(golden, name):
    """[0, S) in one launch == [0, k) then [k, S) from the carried state, bit for bit: hout, hc_last, both saved images; d_pre, d_hh,
    d_h0, d_c0 of the backward.  The range partials are fp64 sums whose grouping differs between the two (per thread over the steps of
    a launch, then over the workgroup): equal to 1e-12 of the sum of magnitudes as fp64, and equal once flushed to fp32."""
    from fqss_amd import kernels as K
    L, H, x = _chain_case(name, golden)
    wih, bih, whh, bhh, ranges = _kernel_operands(L)
    S, B, _ = x.shape
    pre = K.rowlin_fwd(x, wih, bih)
    gout = torch.randn(S, B, 2 * H, generator=torch.Generator().manual_seed(3)).cuda()
    new_gaccs = lambda: [torch.zeros(K.GACC_DOUBLES, dtype=torch.float64, device="cuda") for _ in range(23)] + [None]

    def flushed(gaccs):
        sums = torch.stack([a.view(-1, 3).sum(0) for a in gaccs[:23]])
        mags = torch.stack([a.view(-1, 3).abs().sum(0) for a in gaccs[:23]])
        out = torch.zeros(23, 2, device="cuda")
        for i, a in enumerate(gaccs[:23]):
            K.gacc_flush(a, out[i, 0:1], out[i, 1:2], None)
        return sums, mags, out

    hout, hc, hsav, csav = K.lstmq_fwd(pre, whh, bhh, ranges, S, B, H, want_last=True)
    ga = new_gaccs()
    d_pre, d_hh, d_h0, d_c0 = K.lstmq_bwd(gout, whh, pre, hsav, csav, ranges, ga, S, B, H, want_state=True)
    sums, mags, fl = flushed(ga)
    assert all(torch.isfinite(t).all() for t in (hout, hc, hsav, csav, d_pre, d_hh, d_h0, d_c0))
    assert float(sums[:, :2].abs().min()) > 0 or S * B < 4
    for k in sorted({1, 3, S - 1} & set(range(1, S))):
        h1, hc1, hs1, cs1 = K.lstmq_fwd(pre, whh, bhh, ranges, S, B, H, k0=0, k1=k, want_last=True)
        h2, hc2, hs2, cs2 = K.lstmq_fwd(pre, whh, bhh, ranges, S, B, H, k0=k, k1=S, h0=hc1[0].contiguous(), c0=hc1[1].contiguous(), out=(h1, hs1, cs1),
                                        want_last=True)
        for a, b, what in ((h2, hout, "hout"), (hc2, hc, "hc_last"), (hs2, hsav, "hsav"), (cs2, csav, "csav")):
            assert torch.equal(a, b), (name, k, what)
        gb = new_gaccs()
        p2, q2, dh, dc = K.lstmq_bwd(gout, whh, pre, hsav, csav, ranges, gb, S, B, H, k0=k, k1=S, c0=hc1[1].contiguous(), want_state=True)
        p1, q1, dh0, dc0 = K.lstmq_bwd(gout, whh, pre, hsav, csav, ranges, gb, S, B, H, k0=0, k1=k, g_hc_last=torch.stack([dh, dc]).contiguous(),
                                       want_state=True, out=(p2, q2))
        for a, b, what in ((p1, d_pre, "d_pre"), (q1, d_hh, "d_hh"), (dh0, d_h0, "d_h0"), (dc0, d_c0, "d_c0")):
            assert torch.equal(a, b), (name, k, what)
        s2, _, f2 = flushed(gb)
        assert bool(((s2 - sums).abs() <= 1e-12 * mags).all()), (name, k)
        assert torch.equal(f2, fl), (name, k)
    if S == 1:      # (no interior split point: the single step from a carried state instead, against the same step of a 2-step run)
        x2 = torch.cat([x, x], 0)
        pre2 = K.rowlin_fwd(x2, wih, bih)
        _, hc_a, _, _ = K.lstmq_fwd(pre2, whh, bhh, ranges, 2, B, H, k0=0, k1=1, want_last=True)
        full = K.lstmq_fwd(pre2, whh, bhh, ranges, 2, B, H, want_last=True)
        part = K.lstmq_fwd(pre2, whh, bhh, ranges, 2, B, H, k0=1, k1=2, h0=hc_a[0].contiguous(), c0=hc_a[1].contiguous(), want_last=True)
        assert torch.equal(full[1], part[1]) and torch.equal(full[0][1, :, :H], part[0][1, :, :H]) and torch.equal(full[0][0, :, H:], part[0][0, :, H:])


# ------------------------------------------------------------------------- 2b. H = 128: the register-resident forward against the generic
def _codes(v, rng):
    lo, hi = rng[0].item(), rng[1].item()
    return np.clip(np.rint((v.double().cpu().numpy() - lo) / ((hi - lo) / 255.0)), 0, 255)


def _g1_codes(a, b, what):
    frac, dmax = float(np.mean(a != b)), float(np.abs(a - b).max())
    print(f"{what}: differing fraction {frac:.3e}, largest index distance {dmax:.0f}")
    assert dmax <= 1 and frac <= 2e-3, (what, frac, dmax)
    return int((a != b).sum())


@pytest.mark.parametrize("name", ["h128", "h128s1"])
def test_h128_specialised_forward_against_generic(golden, name, monkeypatch):
    """k_lstmq_fwd_st<128> in ONE free-running launch against the generic kernel (kernels.LSTMQ_GENERIC_FWD) teacher-forced step by
    step from the specialised launch's own carried state, so that one flipped bin cannot cascade: every step's h (hout, mul2 grid), c
    (csav, add1 grids; sequence 1's is written half a step late by the specialised form) and W_hh h + b_hh (hsav: on fq_hh's grid, and
    as floats within the bound of two fp32 sums of H + 1 terms in different orders), hc_last; then the 512-thread backward on either
    set of saved images: d_pre, d_hh and the flushed range gradients by the `gin` rule with its flip allowance."""
    from fqss_amd import kernels as K
    L, H, x = _chain_case(name, golden)
    wih, bih, whh, bhh, ranges = _kernel_operands(L)
    S, B, _ = x.shape
    site = lambda s, d: ranges[d * 12 + K.LSTMQ_SITES.index(s)]
    pre = K.rowlin_fwd(x, wih, bih)
    hout, hc, hsav, csav = K.lstmq_fwd(pre, whh, bhh, ranges, S, B, H, want_last=True)
    monkeypatch.setattr(K, "LSTMQ_GENERIC_FWD", True)
    ref = tuple(torch.zeros_like(t) for t in (hout, hsav, csav))
    hc_ref = None
    for k in range(S):
        state = {}
        if k > 0:       # the state after step k-1: time k-1 forward, time S-k reverse
            state = dict(h0=torch.stack([hout[k - 1, :, :H], hout[S - k, :, H:]]).contiguous(),
                         c0=torch.stack([csav[k - 1, :, 0], csav[S - k, :, 1]]).contiguous())
        _, hc_ref, _, _ = K.lstmq_fwd(pre, whh, bhh, ranges, S, B, H, k0=k, k1=k + 1, out=ref, want_last=True, **state)
    monkeypatch.setattr(K, "LSTMQ_GENERIC_FWD", False)
    torch.cuda.synchronize()
    g_h, g_hs, g_cs = ref
    nflip = _g1_codes(_codes(hout, site("mul2", 0)), _codes(g_h, site("mul2", 0)), f"{name} hout")
    _g1_codes(_codes(hc[0], site("mul2", 0)), _codes(hc_ref[0], site("mul2", 0)), f"{name} hc_last h")
    hs4, gs4 = hsav.view(S, B, 2, 4 * H), g_hs.view(S, B, 2, 4 * H)
    for d, sfx in ((0, "forward"), (1, "reverse")):
        nflip += _g1_codes(_codes(csav[:, :, d], site("add1", d)), _codes(g_cs[:, :, d], site("add1", d)), f"{name} csav {sfx}")
        _g1_codes(_codes(hc[1, d], site("add1", d)), _codes(hc_ref[1, d], site("add1", d)), f"{name} hc_last c {sfx}")
        nflip += _g1_codes(_codes(hs4[:, :, d], site("hh", d)), _codes(gs4[:, :, d], site("hh", d)), f"{name} hsav {sfx}")
        hp = torch.zeros(S, B, H, device="cuda", dtype=torch.float64)          # h of the step before, by time
        if S > 1 and d == 0:
            hp[1:] = hout[:-1, :, :H].double()
        elif S > 1:
            hp[:-1] = hout[1:, :, H:].double()
        bound = 2 * (H + 1) * 2.0 ** -24 * (hp.abs() @ whh[d].double().abs().T + bhh[d].double().abs())
        assert bool(((hs4[:, :, d].double() - gs4[:, :, d].double()).abs() <= bound).all()), (name, sfx)
    # the backward on the specialised forward's images and on the generic forward's
    gout = torch.randn(S, B, 2 * H, generator=torch.Generator().manual_seed(3)).cuda()
    res = []
    for hs_, cs_ in ((hsav, csav), (g_hs, g_cs)):
        ga = [torch.zeros(K.GACC_DOUBLES, dtype=torch.float64, device="cuda") for _ in range(23)] + [None]
        d_pre, d_hh, _, _ = K.lstmq_bwd(gout, whh, pre, hs_, cs_, ranges, ga, S, B, H)
        fl = torch.zeros(23, 2, device="cuda")
        for i, a in enumerate(ga[:23]):
            K.gacc_flush(a, fl[i, 0:1], fl[i, 1:2], None)
        res.append((d_pre, d_hh, fl))
    for a, b, what in zip(res[0], res[1], ("d_pre", "d_hh", "range gradients")):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.isfinite(a).all() and float(np.abs(a).max()) > 0, what
        bad = np.abs(a - b) > (1e-4 + 1e-4 * np.abs(b))
        assert bad.mean() <= 2e-3 + 4.0 * nflip / a.size, (name, what, bad.mean(), nflip)


def test_backward_range_partials_past_the_slot_count():
    """more workgroups than FQSS_GACC_SLOTS (over 2048 sequences): the partials fold onto the slots; the sums are those of the same
    sequences run in blocks of 1024 that each have their own slots.  Bound: a quantizer's sum has N <= S B 2 (4H) = 5.3e5 fp32 terms
    added in fp64 in two groupings, each within N 2^-53 = 6e-11 of the terms' magnitude sum; that sum is not known here, but a slot
    holds >= 64 terms of either sign, so it is below ~ sqrt(64) x 4 = 32 times the slots' magnitude sum: 2 x 6e-11 x 32 = 4e-9 of the
    latter (a lost or misplaced workgroup partial would be an error of 1 / 2050 of it)."""
    from fqss_amd import kernels as K
    H, S, B = 8, 2, 4100
    assert 2 * ((B + 1) // 2) > K.GACC_DOUBLES // 3
    L, gen = _random_layer(H, 9)
    wih, bih, whh, bhh, ranges = _kernel_operands(L)
    x = torch.randn(S, B, I_DIM, generator=gen).cuda()
    gout = torch.randn(S, B, 2 * H, generator=gen).cuda()
    new = lambda: [torch.zeros(K.GACC_DOUBLES, dtype=torch.float64, device="cuda") for _ in range(23)] + [None]

    def run(xs, gs, ga):
        pre = K.rowlin_fwd(xs.contiguous(), wih, bih)
        _, _, hsav, csav = K.lstmq_fwd(pre, whh, bhh, ranges, S, xs.shape[1], H)
        return K.lstmq_bwd(gs.contiguous(), whh, pre, hsav, csav, ranges, ga, S, xs.shape[1], H)[:2]

    ga = new()
    d_pre, d_hh = run(x, gout, ga)
    gb = new()
    parts = [run(x[:, lo:lo + 1024], gout[:, lo:lo + 1024], gb) for lo in range(0, B, 1024)]
    assert torch.equal(d_pre, torch.cat([p[0] for p in parts], 1)) and torch.equal(d_hh, torch.cat([p[1] for p in parts], 1))
    for i in range(23):
        a, b = ga[i].view(-1, 3), gb[i].view(-1, 3)
        mag = torch.maximum(a.abs().sum(0), b.abs().sum(0))
        assert float(mag[:2].min()) > 0 and bool(((a.sum(0) - b.sum(0)).abs() <= 4e-9 * mag).all()), i


# --------------------------------------------------------------------------------- 4. free-running forward + backward against the fixture
def test_module_forward_backward_against_reference(golden):
    g = golden("lstmq_static")
    L, H = _fixture_layer(g, "q8")
    _leave_observer(L)
    x = T(g["q8.x"]).cuda().requires_grad_(True)
    y = L(x)[0]
    y.backward(T(g["q8.gout"]).cuda())
    out, ref = y.detach().cpu().numpy(), g["q8.out"]
    _g1(out, ref, *_rng(g, "q8", "activation_fake_quantize"), "layer output")
    nflip = int((np.abs(out - ref) > 1e-6).sum())
    gin = x.grad.cpu().numpy()
    bad = np.abs(gin - g["q8.gin"]) > (1e-4 + 1e-4 * np.abs(g["q8.gin"]))
    assert bad.mean() <= 2e-3 + 4.0 * nflip / gin.size, bad.mean()
    params = dict(L.named_parameters())
    seen = 0
    for k in g.files:
        if not k.startswith("q8.grad."):
            continue
        name = k[len("q8.grad."):]
        p, ref_g = params[name], g[k]
        assert p.grad is not None, name
        got = p.grad.cpu().numpy()
        tol = 2e-3 * (np.abs(ref_g).max() + 1e-6) + 0.02 * nflip * np.abs(ref_g).max()
        np.testing.assert_allclose(got, ref_g, rtol=2e-3, atol=tol, err_msg=name)
        if name.startswith("activation_fake_quantize_"):
            assert float(np.abs(got).max()) > 0, name
            seen += 1
    assert seen == 46
    for r in (L.activation_fake_quantize_mul2_r.min_range, L.activation_fake_quantize_mul2_r.max_range):
        assert r.grad is None or float(r.grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------ 5. fused against stepwise
@pytest.mark.parametrize("name", ["q8", "q24", "h128", "h128s1", "h136"])
def test_fused_against_stepwise(golden, name, monkeypatch):
    """the same module and input through ops_dp.LstmBiQ and, FUSE_LSTMQ off, step by step: outputs within G1; where they are bit-equal,
    gradients agree within 1e-4 + 1e-4 |g| on all but 2e-3 of the elements (the `gin` rule of test_layer_goldens_teacher_forced)"""
    from fqss_amd import ops_dp
    from fqss_amd.quantization.qat import qat_layers as QL
    if name in ("q8", "q24"):
        g = golden("lstmq_static")
        L, H = _fixture_layer(g, name)
        _leave_observer(L)
        x0 = T(g[f"{name}.x"]).cuda()
    else:
        L, H, x0 = _chain_case(name, golden)
    gout = torch.randn(*x0.shape[:2], 2 * H, generator=torch.Generator().manual_seed(11)).cuda()

    def run():
        L.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = L(x)[0]
        y.backward(gout)
        return y.detach(), [x.grad] + [p.grad for _, p in sorted(L.named_parameters()) if p.grad is not None]

    n0 = ops_dp.LSTMQ_LAUNCHES
    y1, g1 = run()
    assert ops_dp.LSTMQ_LAUNCHES == n0 + 1
    monkeypatch.setattr(QL, "FUSE_LSTMQ", False)
    y2, g2 = run()
    assert ops_dp.LSTMQ_LAUNCHES == n0 + 1
    aq = L.activation_fake_quantize
    _g1(y1.cpu().numpy(), y2.cpu().numpy(), aq.min_range.item(), aq.max_range.item(), f"{name} fused vs stepwise")
    assert len(g1) == len(g2) and len(g1) >= 1 + 8 + 46
    # bit-equal outputs (nflip = 0): the rule as it stands; otherwise with that test's allowance per differing output element
    nflip = int((y1 != y2).sum())
    print(f"{name}: outputs differ in {nflip} of {y1.numel()} elements")
    for a, b in zip(g1, g2):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        bad = np.abs(a - b) > (1e-4 + 1e-4 * np.abs(b))
        assert bad.mean() <= 2e-3 + 4.0 * nflip / a.size, (name, a.shape, bad.mean(), nflip)


# ------------------------------------------------------------------------------------------------------- 7. through the public surface
def test_static_lstm_through_trainer_resume_and_serving(tmp_path, monkeypatch):
    """configs/dptnet_2spks_8k_synthetic_lstmq.yaml through the asteroid env (the sizes of tests/test_gpu_env.py's DPTNet run: 56 steps,
    the 50-call observer phase of the other layers ends inside epoch 4; the step quantizers leave theirs inside the first forward):
    finite losses, the captured step replays, checkpoint.pth resumes with the step quantizers' state as stored; the trained model serves
    through InferRunner's graph with the bits of the eager eval forward (carriers NaN-poisoned by the suite's fixture)."""
    import os
    import yaml
    from fqss_amd import checkpoint, ops
    from fqss_amd.quantization.qat import qat_layers as QL
    from fqss_amd.quantization.qat.models.load_model import create_pretrained_model, enable_observer
    from fqss_amd.runtime import InferRunner
    from fqss_amd.train_env.asteroid_librimix import asteroid_librimix_trainer as A
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    conf = yaml.safe_load(open(os.path.join(root, "configs", "dptnet_2spks_8k_synthetic_lstmq.yaml")))
    conf["work_dir"] = str(tmp_path / "run")
    conf["dataset_cfg"].update(segment=0.25, steps_per_epoch=14, val_steps=1)

    def train(epochs, resume=None):
        conf["training_cfg"].update(epochs=epochs)
        if resume is not None:
            conf["training_cfg"]["resume"] = resume
        yml = tmp_path / f"cfg{epochs}.yaml"
        yml.write_text(yaml.safe_dump(conf))
        return A.train(str(yml), "cuda")

    hist = train(4)
    assert len(hist) == 4 and all(np.isfinite(h["loss"]) and np.isfinite(h["val_loss"]) for h in hist)
    assert [h["launch"] for h in hist] == ["eager", "eager", "eager", "hipGraph replay"]
    path = os.path.join(conf["work_dir"], "checkpoint.pth")
    ck = checkpoint.load_training_state(path)
    assert ck["format"] == checkpoint.FORMAT == "fqss-train-v1"
    aq = ck["step"]["act_quantizers"]
    lstm = "separator.DPT.row_transformer.0.transformer.lstm.activation_fake_quantize_"
    assert aq[lstm + "hh"]["n_iter"] == 50 and aq[lstm + "mul2"]["n_iter"] == 50 and aq[lstm + "mul2_r"]["n_iter"] == 0
    # what the file holds for every LSTM step quantizer, and what the resumed run holds BEFORE its first step
    lay = ck["step"]["arena"]["layout"]
    stored = {n: ck["step"]["arena"]["flat_p"][o:o + m].clone() for n, o, m in zip(lay["names"], lay["offsets"], lay["numel"])
              if ".lstm.activation_fake_quantize_" in n}
    assert len(stored) == 12 * 24 * 2 and float(stored[lstm + "hh.min_range"]) != -0.5 and float(stored[lstm + "mul2_r.min_range"]) == -0.5
    seen = {}
    restore = checkpoint.restore

    def spy(ckpt, step, teacher):
        out = restore(ckpt, step, teacher)
        from fqss_amd.quantization.qat.qat_quant import GradientActivationFakeQuantize
        seen["ranges"] = {n: p.detach().cpu().clone() for n, p in step.model.named_parameters() if n in stored}
        seen["n_iter"] = {n: m.n_iter for n, m in step.model.named_modules() if isinstance(m, GradientActivationFakeQuantize)}
        return out

    monkeypatch.setattr(checkpoint, "restore", spy)
    hist5 = train(5, resume="auto")
    monkeypatch.setattr(checkpoint, "restore", restore)
    assert set(seen["ranges"]) == set(stored) and all(torch.equal(seen["ranges"][n], stored[n]) for n in stored)
    assert seen["n_iter"] == {k: v["n_iter"] for k, v in aq.items()}
    assert len(hist5) == 5 and hist5[:4] == hist and np.isfinite(hist5[4]["loss"]) and hist5[4]["launch"] == "hipGraph replay"
    ck5 = checkpoint.load_training_state(path)
    assert ck5["format"] == ck["format"] and {k: v["n_iter"] for k, v in ck5["step"]["act_quantizers"].items()} == {k: v["n_iter"] for k, v in aq.items()}
    # serving
    model_cfg = dict(conf["model_cfg"], model_path=os.path.join(conf["work_dir"], "best_model.pth"))
    model = create_pretrained_model(model_cfg).cuda().eval()
    enable_observer(model, False)
    assert sum(isinstance(m, QL.LSTMQ_static) for m in model.modules()) == 12
    sd = model.state_dict()
    assert float(sd[lstm + "mul2_r.min_range"]) == -0.5 and float(sd[lstm + "hh.min_range"]) != -0.5
    x = torch.randn(1, 2000, generator=torch.Generator().manual_seed(1)).cuda()
    with ops.poison_carriers(True):
        with torch.no_grad():
            want = model(x)
        run = InferRunner(model)
        got = run(x).clone()
        assert len(run._graphs) == 1 and torch.isfinite(want).all() and torch.equal(got, want)
        assert torch.equal(run(x), want)


# --------------------------------------------------------------------------------------------------------------------- 6. calibration
def test_calibration_counts_time_steps(golden, monkeypatch):
    """observer on, first forward of S = 56 steps: the step quantizers observe 50 time steps (mul2: 25, called by both directions) and
    quantize the rest of the SAME forward; ranges within 1e-5 relative of the reference's, n_iter equal, mul2_r untouched.  The second
    forward has an empty prefix: one fused launch, no step-by-step call."""
    from fqss_amd import ops_dp
    from fqss_amd.quantization.qat import qat_layers as QL
    g = golden("lstmq_static")
    L, H = _fixture_layer(g, "cal")
    # the checkpoint holds the ranges AFTER calibration: start from a fresh module's, as the generator did
    from fqss_amd.quantization.qat import qat_quant as QQ
    with torch.no_grad():
        for m in L.modules():
            if isinstance(m, (QQ.GradientActivationFakeQuantize, QQ.GradientWeightFakeQuantize)):
                m.min_range.fill_(-0.5)
                m.max_range.fill_(0.5)
    x = T(g["cal.x"]).cuda()
    S = x.shape[0]
    calls = []
    step = QL._lstmq_step
    monkeypatch.setattr(QL, "_lstmq_step", lambda *a, **k: (calls.append(1), step(*a, **k))[1])
    n0 = ops_dp.LSTMQ_LAUNCHES
    with torch.no_grad():
        y = L(x)[0]
    assert len(calls) == 2 * 50 and ops_dp.LSTMQ_LAUNCHES == n0 + 1
    for name, n_ref in zip(g["cal.quantizers"], g["cal.n_iter"]):
        q = getattr(L, str(name))
        assert q.n_iter == int(n_ref), name
        for r in ("min_range", "max_range"):
            ref = float(g[f"cal.sd.{name}.{r}"][0])
            assert abs(getattr(q, r).item() - ref) <= 1e-5 * abs(ref), (name, r, getattr(q, r).item(), ref)
    q = L.activation_fake_quantize_mul2_r
    assert q.n_iter == 0 and q.min_range.item() == -0.5 and q.max_range.item() == 0.5
    # the output: un-quantized floats for the steps mul2 observed (k < 25), values on mul2's grid afterwards
    out, ref = y.cpu().numpy(), g["cal.out"]
    lo, hi = _rng(g, "cal", "activation_fake_quantize_mul2")
    k_f = np.arange(S)[:, None, None] * np.ones((1, out.shape[1], H), dtype=np.int64)
    step_of = np.concatenate([k_f, S - 1 - k_f], -1)
    fl = step_of < 25
    np.testing.assert_allclose(out[fl], ref[fl], rtol=1e-5, atol=1e-6)
    _g1(out[~fl], ref[~fl], lo, hi, "calibration forward, quantized steps")
    calls.clear()
    with torch.no_grad():
        L(x)
    assert calls == [] and ops_dp.LSTMQ_LAUNCHES == n0 + 2
