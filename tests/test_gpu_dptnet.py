"""GPU parity of the dual-path (DPTNet, SURVEY.md §8 row a13 / cfg 3) product path -- modules -> ops_dp -> C ABI -> HIP --
against the oracle (oracle/dptnet_oracle.py) and the reference-generated fixtures (tests/golden/dpt_*.npz, cfg3_step.npz):
kernels vs CPU float math, every new LayerQ teacher-forced with the reference's input, the 50-call observers, the tiny
model's QAT steps (free-running and from the reference's own states), the float teacher, and the full-size network."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import oracle.dptnet_oracle as D
import oracle.fqss_oracle as O

pytestmark = pytest.mark.gpu

TINY = dict(n_spks=2, kernel_size=2, enc_dim=16, feature_dim=8, hidden_dim=12, layer=2, segment_size=10)
TINY_O = dict(n_src=2, kernel_size=2, segment_size=10)
QCFG = {"qat": True, "gradient_based": True, "weight_quant": True, "weight_n_bits": 8, "act_quant": True, "act_n_bits": 8,
        "in_quant": False, "in_act_n_bits": 8, "out_quant": True, "out_act_n_bits": 8, "n_splitter": 2, "n_combiner": 2,
        "observer": True}
P = dict(gradient_based=True, weight_quant=True, act_quant=True, act_n_bits=8, weight_n_bits=8)
A = dict(gradient_based=True, act_quant=True)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    yield


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def close(got, want, rtol=2e-5, atol=None, msg=""):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    atol = atol if atol is not None else rtol * float(want.abs().max())
    err = float((got - want).abs().max())
    assert err <= atol + rtol * float(want.abs().max()), (msg, err, float(want.abs().max()))


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("R,Ci,Co", [(45, 24, 16), (1000, 64, 192), (777, 256, 64), (300, 64, 1024), (129, 16, 2)])
def test_rowlin_kernels(R, Ci, Co):
    from fqss_amd import kernels as K
    x, w, b, g = rnd(R, Ci, seed=1), rnd(Co, Ci, seed=2, scale=0.2), rnd(Co, seed=3), rnd(R, Co, seed=4)
    xd, wd, bd, gd = x.cuda(), w.cuda(), b.cuda(), g.cuda()
    close(K.rowlin_fwd(xd, wd, bd), x.double() @ w.double().T + b.double(), 3e-6)
    close(K.rowlin_bwd_x(gd, wd), g.double() @ w.double(), 3e-6)
    gw = torch.zeros(Co, Ci, device="cuda")
    K.rowlin_bwd_w(gd, xd, gw)
    close(gw, g.double().T @ x.double(), 5e-6)
    gb = torch.zeros(Co, device="cuda")
    K.colsum(gd, gb)
    close(gb, g.double().sum(0), 5e-6)
    # column-block views (the LSTM / attention paths write and read sub-blocks of wider buffers)
    wide = torch.zeros(R, 3 * Co, device="cuda")
    K.rowlin_fwd(xd, wd, bd, out=wide[:, Co:2 * Co])
    close(wide[:, Co:2 * Co], x.double() @ w.double().T + b.double(), 3e-6)
    assert float(wide[:, :Co].abs().max()) == 0 and float(wide[:, 2 * Co:].abs().max()) == 0


@pytest.mark.parametrize("S,B,H", [(9, 5, 12), (250, 3, 128), (33, 4, 64)])
def test_rowlin_bwd_w_pair_on_shifted_views(S, B, H, monkeypatch):
    """the two directions' W_hh gradients of a bidirectional LSTM in one batched launch == two launches == fp64"""
    from fqss_amd import kernels as K
    dG, h = rnd(S, B, 8 * H, seed=5), rnd(S, B, 2 * H, seed=6)
    dGd, hd = dG.cuda(), h.cuda()
    want = [(dG[1:, :, :4 * H].double().reshape(-1, 4 * H).T @ h[:-1, :, :H].double().reshape(-1, H)),
            (dG[:-1, :, 4 * H:].double().reshape(-1, 4 * H).T @ h[1:, :, H:].double().reshape(-1, H))]
    for on in (True, False):
        monkeypatch.setattr(K, "PAIR_WGRAD", on)
        flat = torch.zeros(3 * 4 * H * H + 8, device="cuda")
        g0, g1 = flat[:4 * H * H].view(4 * H, H), flat[2 * 4 * H * H + 8:].view(4 * H, H)       # two slots of one arena, a gap between them
        K.rowlin_bwd_w_pair(dGd[1:, :, :4 * H], hd[:-1, :, :H], g0, dGd[:-1, :, 4 * H:], hd[1:, :, H:], g1)
        close(g0, want[0], 5e-6, msg=f"fwd dir, pair={on}")
        close(g1, want[1], 5e-6, msg=f"rev dir, pair={on}")
        assert float(flat[4 * H * H:2 * 4 * H * H + 8].abs().max()) == 0


@pytest.mark.parametrize("C", [8, 16, 64, 200])
def test_layernorm_kernels(C):
    from fqss_amd import kernels as K
    x = (rnd(7, 33, C, seed=5) * 1.7 + 0.3).requires_grad_(True)
    ga, be = (1 + 0.1 * rnd(C, seed=6)).requires_grad_(True), (0.1 * rnd(C, seed=7)).requires_grad_(True)
    y = F.layer_norm(x, (C,), ga, be, 1e-5)
    g = rnd(7, 33, C, seed=8)
    y.backward(g)
    yd, ms = K.layernorm_fwd(x.detach().cuda(), ga.detach().cuda(), be.detach().cuda(), 1e-5)
    close(yd, y, 3e-6)
    gg, gb = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    gx = K.layernorm_bwd(g.cuda(), x.detach().cuda(), ga.detach().cuda(), ms, gg, gb)
    close(gx, x.grad, 1e-5)
    close(gg, ga.grad, 1e-5)
    close(gb, be.grad, 1e-5)


def test_unary_and_data_movement_kernels(golden):
    from fqss_amd import kernels as K
    from fqss_amd import ops_dp
    x = rnd(5, 1000, seed=9, scale=2.0)
    for kind, fn in ((K.UNARY_TANH, torch.tanh), (K.UNARY_SIGMOID, torch.sigmoid)):
        xr = x.clone().requires_grad_(True)
        y = fn(xr)
        g = rnd(5, 1000, seed=10)
        y.backward(g)
        yd = K.unary_fwd(x.cuda(), kind)
        close(yd, y, 3e-7, atol=3e-7)
        close(K.unary_bwd(g.cuda(), yd, kind), xr.grad, 1e-6, atol=1e-6)
    s = float(np.sqrt(2.0))
    assert torch.equal(K.unary_fwd(x.cuda(), K.UNARY_DIVS, s).cpu(), x / s)          # IEEE division, bit-exact
    gl = golden("dpt_layers")
    # split_feature / merge_feature / overlap_and_add against the reference's own outputs
    for Tn in (37, 40, 45):
        f = T(gl[f"seg{Tn}.in"])
        B, N, _ = f.shape
        seg_ref = T(gl[f"seg{Tn}.out"])                       # [B, N, K, S]
        Kc, S = seg_ref.shape[2], seg_ref.shape[3]
        fd = f.cuda().requires_grad_(True)
        seg = ops_dp.Segment.apply(fd, Kc)                    # [K, B*S, N]
        assert torch.equal(seg.detach().cpu().view(Kc, B, S, N).permute(1, 3, 0, 2), seg_ref)
        cols = ops_dp.rows_to_cols(seg, B, S)                 # [S, B*K, N]
        assert torch.equal(cols.detach().cpu().view(S, B, Kc, N).permute(1, 3, 2, 0), seg_ref)
        back = ops_dp.cols_to_rows(cols, B, Kc)
        assert torch.equal(back.detach(), seg.detach())
        # merge with nspk = 1: o[s][b*K+k][n] = seg
        a, b = ops_dp.MergeStreams.apply(cols, B, 1, N, Kc)
        rest = int(gl[f"seg{Tn}.rest"])
        m = (a + b)[:, :, :Tn]
        assert torch.equal(m.detach().cpu().view(B, N, Tn), T(gl[f"seg{Tn}.merged"]))
        gm = rnd(*a.shape, seed=11).cuda()
        (a * gm).sum().backward()
        fr = f.clone().requires_grad_(True)
        sr, _ = D.split_feature(fr, Kc)
        ar, _ = D.merge_halves(sr)
        (ar * gm.cpu().view(ar.shape)).sum().backward()
        close(fd.grad, fr.grad, 1e-6)
    sig = T(gl["ola.in"])[..., :2].contiguous()                # [2, 3, 11, 2]
    from fqss_amd.quantization.qat.models.dptnetq import overlap_and_add
    sd = sig.cuda().requires_grad_(True)
    out = overlap_and_add(sd, 1)
    assert torch.equal(out.detach().cpu(), T(gl["ola.out_step1"]))
    g = rnd(*out.shape, seed=12)
    out.backward(g.cuda())
    sr = sig.clone().requires_grad_(True)
    D.overlap_and_add(sr, 1).backward(g)
    close(sd.grad, sr.grad, 1e-7)


@pytest.mark.parametrize("L,B,nh,hd", [(9, 5, 4, 4), (250, 6, 4, 16), (194, 3, 4, 16), (37, 4, 4, 2), (300, 2, 8, 32), (250, 3, 8, 32), (34, 5, 8, 32),
                                       (256, 2, 4, 16), (33, 2, 4, 16)])
def test_attention_kernels(L, B, nh, hd):
    """K.attn_fwd / K.attn_bwd against the oracle's fp32 attention core.  Which kernels a case runs is the dispatcher's choice
    (kernels._attn_stream_ok; pinned by test_attention_dispatch below): q dense, k / v column blocks of an [L, B, 3E] buffer with E a
    multiple of 16 are 16-B aligned views, so the seven cases with head_dim 16 / 32 run the streaming kernels of csrc/attn_long.hip
    (fqss_attn_long_fwd / _bwd, as test_attn_long does); only (9, 5, 4, 4) and (37, 4, 4, 2) run the LDS-resident kernels of
    csrc/attn.hip (k_attn_fwd<4>, <2>, k_attn_bwd<4>, <2>).  The LDS-resident family has its own test against float64 at every head
    width and kernel form: tests/test_gpu_sequence_kernels.py."""
    from fqss_amd import kernels as K
    E = nh * hd
    X = rnd(L, B, 3 * E, seed=13, scale=0.8)
    q = (X[..., :E] / np.sqrt(hd)).clone().requires_grad_(True)
    k, v = X[..., E:2 * E].clone().requires_grad_(True), X[..., 2 * E:].clone().requires_grad_(True)
    ref = D.mha_core(q * np.sqrt(hd), k, v, nh)                      # mha_core divides by sqrt(hd) itself
    g = rnd(L, B, E, seed=14)
    ref.backward(g)
    Xd = X.cuda()
    qd = q.detach().cuda()
    ws = torch.tensor([-1, 0, -1, 0], dtype=torch.int32, device="cuda")
    o, st = K.attn_fwd(qd, Xd[..., E:2 * E], Xd[..., 2 * E:], L, B, nh, ws[:2], ws[2:])
    close(o, ref, 5e-6)
    gq, gk, gv = K.attn_bwd(qd, Xd[..., E:2 * E], Xd[..., 2 * E:], o, g.cuda(), st, L, B, nh)
    close(gq, q.grad, 2e-5)
    close(gk, k.grad, 2e-5)
    close(gv, v.grad, 2e-5)
    # observer side outputs: min / max of the logits and of the probabilities
    qh = q.detach().reshape(L, B * nh, hd).permute(1, 0, 2)
    kh = k.detach().reshape(L, B * nh, hd).permute(1, 0, 2)
    s = torch.bmm(qh, kh.transpose(1, 2))
    p = torch.softmax(s, -1)
    w = ws.cpu().numpy().view(np.uint32)

    def dec(u):
        u = int(u)
        u = (u & 0x7fffffff) if (u & 0x80000000) else (~u & 0xffffffff)
        return np.array([u], dtype=np.uint32).view(np.float32)[0]
    np.testing.assert_allclose([dec(w[0]), dec(w[1])], [float(s.min()), float(s.max())], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose([dec(w[2]), dec(w[3])], [float(p.min()), float(p.max())], rtol=1e-4, atol=1e-12)


def test_attention_dispatch(monkeypatch):
    """which C entry K.attn_fwd / K.attn_bwd choose: the streaming kernels (fqss_attn_long_*) for 16-B aligned head_dim-16 views, the
    LDS-resident ones (fqss_attn_*) for head_dim 8, for a view whose base is one float off alignment, and whenever K.ATTN_STREAM is off.
    A change of the predicate then shows up here instead of silently moving test_attention_kernels to another kernel family."""
    from fqss_amd import _lib
    from fqss_amd import kernels as K
    called = []
    real = _lib.call

    def spy(name, *args):
        called.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", spy)

    def entries(L, B, nh, hd, shift=0):
        E = nh * hd
        flat = rnd(L * B * 3 * E + 4, seed=15, scale=0.5).cuda()
        X = flat[shift:shift + L * B * 3 * E].view(L, B, 3 * E)
        q = X[..., :E].contiguous() if shift == 0 else X[..., :E]
        del called[:]
        o, st = K.attn_fwd(q, X[..., E:2 * E], X[..., 2 * E:], L, B, nh)
        K.attn_bwd(q, X[..., E:2 * E], X[..., 2 * E:], o, torch.ones(L, B, E, device="cuda"), st, L, B, nh)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(o).all())
        return [n for n in called if "attn" in n]

    monkeypatch.setattr(K, "ATTN_STREAM", True)
    assert entries(40, 2, 4, 16) == ["fqss_attn_long_fwd", "fqss_attn_long_bwd"]
    assert entries(40, 2, 4, 8) == ["fqss_attn_fwd", "fqss_attn_bwd"]
    assert entries(40, 2, 4, 16, shift=1) == ["fqss_attn_fwd", "fqss_attn_bwd"]
    monkeypatch.setattr(K, "ATTN_STREAM", False)
    assert entries(40, 2, 4, 16) == ["fqss_attn_fwd", "fqss_attn_bwd"]
    assert entries(40, 2, 8, 32) == ["fqss_attn_fwd", "fqss_attn_bwd"]


def test_lstm_gate_functions():
    """the H = 128 recurrence's own sigmoid / tanh (one short chain on the hardware's exp2 / rcp, csrc/lstm.hip gate_fn) against float64:
    <= 4 ulp of the exact value and within 1.2e-7 of it, the limits beyond the range in which the result is not yet 0 / 1 / +-1"""
    from fqss_amd import _lib
    n = 1 << 22
    g = torch.Generator().manual_seed(5)
    x = torch.cat([torch.linspace(-87, 87, n), torch.randn(n, generator=g) * 3, torch.randn(n, generator=g) * 0.2,
                   torch.tensor([0.0, -0.0, 0.36, -0.36, 1e-30, -1e-30])])
    far = torch.tensor([88.0, -88.0, 200.0, -200.0, 1e30, -1e30, float("inf"), -float("inf")])

    def run(v):
        vd = v.cuda()
        sg, th = torch.empty_like(vd), torch.empty_like(vd)
        _lib.call("fqss_lstm_gate_fn", vd.data_ptr(), sg.data_ptr(), th.data_ptr(), vd.numel(), torch.cuda.current_stream().cuda_stream)
        return sg.cpu(), th.cpu()

    sg, th = run(x)
    x64 = x.double()
    for got, want, name in ((sg, torch.sigmoid(x64), "sigmoid"), (th, torch.tanh(x64), "tanh")):
        assert torch.isfinite(got).all(), name
        ulp = torch.clamp(2.0 ** torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -126))), min=2.0 ** -126) * 2.0 ** -23
        err = (got.double() - want).abs() / ulp
        # measured (tools/lstm_gate_err.py): sigmoid <= 3.5 ulp (<= 1.5 for x > 0), tanh <= 2.6 ulp, either within 1.0e-7 of the exact value
        assert float(err.max()) <= 4.0, (name, float(err.max()), float(x[err.argmax()]))
        assert float((got.double() - want).abs().max()) <= 1.2e-7, name
    assert float(th[-6]) == 0.0 and float(th[-5]) == 0.0 and float(sg[-6]) == 0.5
    sg, th = run(torch.tensor([float("nan"), 1.0]))         # a NaN pre-activation stays a NaN in BOTH functions
    assert bool(torch.isnan(sg[0])) and bool(torch.isnan(th[0])) and bool(torch.isfinite(sg[1])) and bool(torch.isfinite(th[1]))
    sg, th = run(far)
    assert th.tolist() == [1.0, -1.0] * 4
    assert sg[0::2].tolist() == [1.0] * 4 and float(sg[1::2].max()) <= 2e-38 and float(sg[1::2].min()) >= 0.0


@pytest.mark.parametrize("S,B,I,H", [(9, 5, 16, 12), (40, 7, 64, 128), (250, 3, 64, 128)])
def test_lstm_kernels(S, B, I, H):
    from fqss_amd import ops_dp
    names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l0_reverse", "weight_hh_l0_reverse",
             "bias_ih_l0_reverse", "bias_hh_l0_reverse")
    W = {}
    for i, n in enumerate(names):
        shape = (4 * H, I) if "weight_ih" in n else (4 * H, H) if "weight_hh" in n else (4 * H,)
        W[n] = rnd(*shape, seed=20 + i, scale=1.0 / np.sqrt(H)).requires_grad_(True)
    x = rnd(S, B, I, seed=30, scale=0.8).requires_grad_(True)
    ref = D.lstm_bidir(x, W)
    # the oracle's cell against torch's own fused LSTM (what the reference calls)
    lstm = nn.LSTM(I, H, 1, bidirectional=True)
    with torch.no_grad():
        for n in names:
            getattr(lstm, n).copy_(W[n])
    close(ref, lstm(x)[0], 2e-6)
    g = rnd(S, B, 2 * H, seed=31)
    ref.backward(g)
    Wd = {n: W[n].detach().cuda().requires_grad_(True) for n in names}
    xd = x.detach().cuda().requires_grad_(True)
    y = ops_dp.LstmBi.apply(xd, Wd["weight_ih_l0"], Wd["weight_hh_l0"], Wd["bias_ih_l0"], Wd["bias_hh_l0"],
                            Wd["weight_ih_l0_reverse"], Wd["weight_hh_l0_reverse"], Wd["bias_ih_l0_reverse"], Wd["bias_hh_l0_reverse"])
    close(y, ref, 5e-6)
    y.backward(g.cuda())
    close(xd.grad, x.grad, 3e-5)
    for n in names:
        close(Wd[n].grad, W[n].grad, 5e-5, msg=n)


# ------------------------------------------------------------------------------------------------ LayerQ fixtures
class First(nn.Module):
    def __init__(self, m, n_in=1):
        super().__init__()
        self.m, self.n_in = m, n_in

    def forward(self, x):
        return self.m(*([x] * self.n_in))[0]


def _build(name, g):
    from fqss_amd.quantization.qat import qat_layers as QL
    sd = {k[len(name) + 4:]: T(g[k]) for k in g.files if k.startswith(name + ".sd.")}
    shp = lambda k: tuple(sd[k].shape)
    dec = dict(n_combiner=2, gradient_based=True, weight_quant=True, weight_n_bits=8, act_quant=True, act_n_bits=8, out_quant=True,
               out_act_n_bits=8)
    if name == "layernormq":
        L = QL.LayerNormQ(nn.LayerNorm(shp("layernorm.weight")[0]), **A)
    elif name == "linearq":
        co, ci = shp("linear.weight"); L = QL.LinearQ(nn.Linear(ci, co), **P)
    elif name == "lstmq":
        h4, i = shp("m.lstm.weight_ih_l0"); L = First(QL.LSTMQ(nn.LSTM(i, h4 // 4, 1, bidirectional=True), **P))
    elif name == "mhaq":
        e = shp("m.mha.out_proj.weight")[0]; L = First(QL.MultiheadAttentionQ(nn.MultiheadAttention(e, 4, dropout=0.0), **P), 3)
    elif name == "conv2dq":
        co, ci = shp("conv2d.weight")[:2]; L = QL.Conv2dQ(nn.Conv2d(ci, co, 1), **P)
    elif name in ("conv1dnlq_tanh", "conv1dnlq_sigmoid"):
        co, ci, _ = shp("conv1d.weight"); L = QL.Conv1dNlQ(nn.Conv1d(ci, co, 1), nn.Tanh() if name.endswith("tanh") else nn.Sigmoid(), **P)
    elif name in ("mulq_same", "mulq_mask"):
        L = QL.MulQ(QL.Mul(), **A)
    elif name == "addq_seq":
        L = QL.AddQ(QL.Add(), **A)
    elif name == "nlq_prelu4":
        L = QL.NlQ(nn.PReLU(), **A)
    elif name == "conv1dencoderq_k2":
        L = QL.Conv1dEncoderQ([nn.Conv1d(1, shp("conv1d.weight")[0], 2, stride=1, bias=False), nn.ReLU()], n_splitter=2, **P)
    elif name == "groupnormq_enc":
        L = QL.GroupNormQ(nn.GroupNorm(1, shp("groupnorm.weight")[0], eps=1e-8), **A)
    elif name == "lineardecoderq":
        w, e = shp("linear.weight"); L = QL.LinearDecoderQ([nn.Linear(e, w, bias=False)], **dec)
    else:
        raise KeyError(name)
    L.load_state_dict(sd, strict=True)
    return L.cuda().train()


def _leave_observer(L):
    from fqss_amd.quantization.qat import qat_quant as QQ
    for m in L.modules():
        if isinstance(m, QQ.GradientActivationFakeQuantize):
            m.n_iter = m.max_observations
        if isinstance(m, QQ.GradientWeightFakeQuantize):
            m.observer_mode = False


DP_LAYERS = ["layernormq", "linearq", "lstmq", "mhaq", "conv2dq", "conv1dnlq_tanh", "conv1dnlq_sigmoid", "mulq_same", "mulq_mask",
             "addq_seq", "nlq_prelu4", "conv1dencoderq_k2", "groupnormq_enc", "lineardecoderq"]


@pytest.mark.parametrize("name", DP_LAYERS)
def test_dpt_layer_goldens_teacher_forced(golden, name):
    """G1: fed the reference's recorded input, every dual-path LayerQ reproduces the reference's quantized output with at most
    a few bin indices off by one, and its input / parameter gradients"""
    g = golden("dpt_layers")
    L = _build(name, g)
    _leave_observer(L)
    ins, i = [], 0
    while f"{name}.in{i}" in g.files:
        ins.append(T(g[f"{name}.in{i}"]).cuda().requires_grad_(True))
        i += 1
    y = L(*ins)
    y.backward(T(g[f"{name}.gout"]).cuda())
    out, ref = y.detach().cpu().numpy(), g[f"{name}.out"]
    sd = {k[2:] if k.startswith("m.") else k: v for k, v in L.state_dict().items()}
    keys = ["activation_fake_quantize"] + (["activation_fake_quantize_residual"] if name == "lineardecoderq" else [])
    nflip = 0
    for ch, key in enumerate(keys):
        lo, hi = float(sd[key + ".min_range"]), float(sd[key + ".max_range"])
        o, r = (out[ch], ref[ch]) if name == "lineardecoderq" else (out, ref)
        delta = (hi - lo) / 255.0
        a, b = np.rint((o - lo) / delta), np.rint((r - lo) / delta)
        assert np.abs(a - b).max() <= 1, (name, key)
        frac = float(np.mean(a != b))
        assert frac <= (6e-3 if name in ("mhaq", "lstmq", "lineardecoderq") else 3e-3), (name, key, frac)
        nflip += int((a != b).sum())
    for i, x in enumerate(ins):
        if f"{name}.gin{i}" in g.files:
            want = g[f"{name}.gin{i}"]
            bad = np.abs(x.grad.cpu().numpy() - want) > (2e-4 * np.abs(want).max() + 2e-4 * np.abs(want))
            assert bad.mean() <= 2e-3 + 8.0 * nflip / want.size, (name, i, bad.mean())
    params = dict(L.named_parameters())
    for k in g.files:
        if k.startswith(name + ".grad."):
            p = params[k[len(name) + 6:]]
            want = g[k]
            tol = (3e-3 + 0.05 * nflip) * (np.abs(want).max() + 1e-6)
            assert p.grad is not None, k
            np.testing.assert_allclose(p.grad.cpu().numpy(), want, rtol=3e-3, atol=tol, err_msg=k)


@pytest.mark.parametrize("name", ["mhaq", "lstmq", "lineardecoderq", "layernormq"])
def test_dpt_observer_phase_matches_reference(golden, name):
    """50 observer calls on one input: the pass-through output and EVERY range of the layer, including the attention
    quantizers whose outputs the reference discards"""
    g = golden("dpt_layers")
    L = _build(name, g)
    sd = L.state_dict()
    for k in sd:
        if k.endswith("min_range"):
            sd[k] = torch.full_like(sd[k], -0.5)
        elif k.endswith("max_range"):
            sd[k] = torch.full_like(sd[k], 0.5)
    L.load_state_dict(sd)
    x = T(g[name + ".in0"]).cuda()
    with torch.no_grad():
        for _ in range(50):
            y = L(x)
    np.testing.assert_allclose(y.cpu().numpy(), g[name + ".out_obs"], rtol=2e-5, atol=2e-6)
    for k, v in L.state_dict().items():
        if k.endswith("_range"):
            np.testing.assert_allclose(v.cpu().numpy(), g[f"{name}.sd_obs.{k}"], rtol=3e-5, atol=3e-6, err_msg=k)


# ------------------------------------------------------------------------------------------------ model
def build_pair(seed=0, **kw):
    from fqss_amd.quantization.qat.models.dptnetq import DPTNetQ
    from fqss_amd.quantization.qat.models.load_model import quantize_model
    torch.manual_seed(seed)
    model = DPTNetQ(**kw)
    fmodel = copy.deepcopy(model)
    model = quantize_model(model, dict(QCFG))
    return model.cuda().train(), fmodel.cuda().eval()


def _tiny_pair(g, prefix="sd0."):
    model, fmodel = build_pair(0, **TINY)
    model.load_state_dict({k[len(prefix):]: T(g[k]) for k in g.files if k.startswith(prefix)}, strict=True)
    fmodel.load_state_dict({k[4:]: T(g[k]) for k in g.files if k.startswith("fsd.")}, strict=True)
    return model, fmodel


def test_dpt_state_dict_layout(golden):
    g = golden("dpt_tiny_step")
    model, fmodel = _tiny_pair(g)
    assert list(model.state_dict().keys()) == list(g["sd_keys"])
    full, _ = build_pair(0)
    assert sum(p.numel() for p in full.parameters()) > 2_000_000


def test_dpt_teacher_forward_matches_oracle():
    """float path (BYPASS kernels) of the full-size network, B = 2, 1 s"""
    _, fmodel = build_pair(1)
    x, _ = O.synth_batch(2, 4000, seed=2)
    with torch.no_grad():
        y = fmodel(x.cuda()).cpu()
    ref = D.TeacherDPTNet({k: v.cpu() for k, v in fmodel.state_dict().items()})(x)
    np.testing.assert_allclose(y.numpy(), ref.numpy(), rtol=1e-4, atol=2e-5 * float(ref.abs().max()))
    # (O.si_sdr_db saturates at 53 dB here: its 1e-8 energy floor against a 2e-3 signal energy) -> relative L2 error instead
    assert float((y - ref).norm() / ref.norm()) < 1e-4


def _check_step(g, p, r, model, loss_rel, est_tol, grad_tol):
    np.testing.assert_allclose(r["loss"].item(), g[p + "loss"], rtol=loss_rel, err_msg=p)
    np.testing.assert_allclose(r["kd"].item(), g[p + "kd"], rtol=loss_rel, err_msg=p)
    np.testing.assert_allclose(r["w"].cpu().numpy(), g[p + "w"], rtol=2.3e-4, err_msg=p)      # = 1e-3 dB of SI-SDR
    np.testing.assert_allclose(r["est"].cpu().numpy(), g[p + "est"], rtol=1e-4, atol=est_tol, err_msg=p)
    np.testing.assert_allclose(r["gnorm"].item(), g[p + "gnorm"], rtol=2e-4, err_msg=p)
    coef = min(1.0, 5.0 / (float(g[p + "gnorm"]) + 1e-6))
    n = 0
    for name, prm in model.named_parameters():
        k = p + "grad." + name
        if k in g.files:
            ref = g[k] / coef
            err = np.linalg.norm(prm.grad.cpu().numpy() - ref) / (np.linalg.norm(ref) + 1e-12)
            assert err <= grad_tol or np.linalg.norm(ref) < 1e-7, (k, err)
            n += 1
        else:
            assert float(prm.grad.abs().max()) == 0.0, name          # reference: grad is None (attn / softmax ranges)
    assert n >= 80


def test_dpt_tiny_training_vs_reference_goldens(golden):
    """53 QAT steps of the tiny DPTNetQ through KDTrainStep vs the REAL reference's run: step 1 (float arithmetic, observers
    recording) at the G2 tolerances of the north star -- loss / KD 1e-5 relative, SI-SDR 1e-3 dB, every gradient; the chaotic
    rest of the run statistically"""
    from fqss_amd.runtime import KDTrainStep
    g = golden("dpt_tiny_step")
    model, fmodel = _tiny_pair(g)
    step = KDTrainStep(model, fmodel, kd_lambda=0.1, lr=4e-4, clip=5.0)
    x, tgt = T(g["x"]).cuda(), T(g["tgt"]).cuda()
    for s in range(1, 54):
        r = step(x, tgt)
        if s == 1:
            np.testing.assert_allclose(r["sisdr"].cpu().numpy().mean(), float(O.si_sdr_db(T(g["s1.est"]), T(g["tgt"]))), atol=1e-3)
            _check_step(g, "s1.", r, model, 1e-5, 3e-6, 2e-3)
            for k in g.files:
                if k.startswith("s1.post_sd.") and k.endswith("_range") and g[k].size == 1:
                    got = model.state_dict()[k[len("s1.post_sd."):]].cpu().numpy()
                    np.testing.assert_allclose(got, g[k], rtol=3e-5, atol=1e-6, err_msg=k)
        elif f"s{s}.loss" in g.files:
            assert abs(r["loss"].item() - float(g[f"s{s}.loss"])) <= 1.5, (s, r["loss"].item(), float(g[f"s{s}.loss"]))
    assert r["loss"].item() < 4.0


def _forced(g, s):
    from fqss_amd.quantization.qat import qat_quant as QQ
    model, fmodel = _tiny_pair(g, prefix=f"s{s}.post_sd.")
    for m in model.modules():
        if isinstance(m, QQ.GradientWeightFakeQuantize):
            m.observer_mode = False
        if isinstance(m, QQ.GradientActivationFakeQuantize):
            m.n_iter = s if s < m.max_observations else m.max_observations
    return model, fmodel


def test_dpt_tiny_step2_from_reference_state(golden):
    """the first forward with fake-quantized weights (all weight-quantizer kinds of the model: conv, linear, in/out projection,
    LSTM matrices, decoder basis, residual encoder), from the reference's own state after step 1: G2 tolerances"""
    from fqss_amd.runtime import KDTrainStep
    g = golden("dpt_tiny_step")
    model, fmodel = _forced(g, 1)
    step = KDTrainStep(model, fmodel, kd_lambda=0.1, lr=4e-4, clip=5.0)
    r = step._fwd_bwd(T(g["x"]).cuda(), T(g["tgt"]).cuda())
    from fqss_amd import kernels as K
    step.arena.sumsq.zero_()
    K.sumsq(step.arena.flat_g, step.arena.sumsq)
    r["gnorm"] = step.arena.sumsq.sqrt().float()
    _check_step(g, "s2.", r, model, 3e-5, 1e-5, 3e-3)


def test_dpt_tiny_step51_from_reference_state(golden):
    """first fully QUANTIZING step from the reference's own state after 50 steps: free-running through every 8-bit quantizer"""
    from fqss_amd import kernels as K
    g = golden("dpt_tiny_step")
    model, fmodel = _forced(g, 50)
    x, tgt = T(g["x"]).cuda(), T(g["tgt"]).cuda()
    with torch.no_grad():
        est, fest = model(x), fmodel(x)
    out, w, sisdr, _ = K.kd_loss(est, fest, tgt, 0.1, want_grad=False)
    np.testing.assert_allclose(fest.cpu().numpy(), g["s51.fest"], rtol=1e-4, atol=3e-6)
    assert abs(out[0].item() - float(g["s51.loss"])) <= 0.1, (out[0].item(), float(g["s51.loss"]))
    sis_ref = float(O.si_sdr_db(T(g["s51.est"]), T(g["tgt"])))
    assert abs(float(sisdr.mean()) - sis_ref) <= 0.2


def test_dpt_tiny_step51_teacher_forced(golden):
    """G1 inside the real network: state after 50 steps, each LayerQ fed the reference's recorded input of step 51"""
    g = golden("dpt_tiny_step")
    model, _ = _forced(g, 50)
    mods = dict(model.named_modules())
    tot = bad = 0
    worst = 0.0
    with torch.no_grad():
        for name in map(str, g["layer_names"]):
            if name.endswith("residual_error_block") or f"s51.act.{name}" not in g.files:
                continue
            mod = mods[name]
            ins, j = [], 0
            while f"s51.actin{j}.{name}" in g.files:
                ins.append(T(g[f"s51.actin{j}.{name}"]).cuda())
                j += 1
            if name.endswith("self_attn"):
                ins = [ins[0]] * 3
            out = mod(*ins)
            out = out[0] if isinstance(out, (list, tuple)) else out
            out, ref = out.cpu().numpy(), g[f"s51.act.{name}"]
            sd = mod.state_dict()
            keys = ["activation_fake_quantize"] + (["activation_fake_quantize_residual"] if name.endswith("basis_signals") else [])
            for ch, key in enumerate(keys):
                o, r = (out[ch], ref[ch]) if len(keys) == 2 else (out, ref)
                lo, hi = float(sd[key + ".min_range"]), float(sd[key + ".max_range"])
                delta = (hi - lo) / 255.0
                a, b = np.rint((o - lo) / delta), np.rint((r - lo) / delta)
                tot += o.size
                bad += int((a != b).sum())
                worst = max(worst, float(np.abs(a - b).max()))
    assert tot > 20000 and worst <= 1, (tot, worst)
    assert bad / tot <= 2e-3, (bad, tot)


def dpt_fill(mod, prefix):
    """restatement of tools/make_goldens_dptnet.py::fill (name-keyed deterministic parameters)"""
    from tests.helpers_cfg1 import keyed_randn
    with torch.no_grad():
        for k, p in mod.named_parameters():
            if k.endswith("min_range") or k.endswith("max_range"):
                continue
            if p.numel() == 1:
                p.fill_(0.25)
            elif p.dim() == 1 and "norm" in k and k.endswith("weight"):
                p.copy_((1.0 + keyed_randn(prefix + k, tuple(p.shape), 0.1)).to(p.device))
            elif p.dim() == 1:
                p.copy_(keyed_randn(prefix + k, tuple(p.shape), 0.05).to(p.device))
            else:
                fan = max(1, int(np.prod(p.shape[1:])))
                p.copy_(keyed_randn(prefix + k, tuple(p.shape), 1.0 / np.sqrt(fan)).to(p.device))


@pytest.mark.parametrize("fixture", ["cfg3_step", "cfg3_full_step"])
def test_dpt_full_size_vs_reference_goldens(golden, fixture):
    """the FULL-SIZE DPTNetQ (6 dual-path layers, 2.8 M parameters) against digests of the real reference's 52-step run from the
    same name-keyed weights: step 1 at G2 tolerances incl. every per-parameter gradient norm, step 2 (weights quantized after
    Adam's sign-like first update) loosely, steps 51-52 (all quantizers live) statistically.  cfg3_step: 1 x 1 s; cfg3_full_step:
    1 x 3 s = the BASELINE workload of cfg 3 (T = 24000, `tools/make_goldens_dptnet.py --only cfg3 --T 24000`)"""
    from fqss_amd.data import synth_batch
    from fqss_amd.runtime import KDTrainStep
    g = golden(fixture)
    B, T_ = int(g["B"]), int(g["T"])
    model, fmodel = build_pair(0)
    dpt_fill(fmodel, "T.")
    dpt_fill(model, "S.")
    assert [k for k, _ in model.named_parameters()] == list(g["param_names"])
    assert [k for k, _ in fmodel.named_parameters()] == list(g["tparam_names"])
    np.testing.assert_allclose([float(p.detach().double().sum()) for _, p in model.named_parameters()], g["param_sum"], rtol=1e-9, atol=1e-9)
    x, tgt = synth_batch(B, T_, seed=0, device="cuda")
    step = KDTrainStep(model, fmodel, kd_lambda=0.1, lr=4e-4, clip=5.0)
    for s in range(1, 53):
        r = step(x, tgt)
        p = f"s{s}."
        if p + "loss" not in g.files:
            continue
        if s <= 2:
            f = 1.0 if s == 1 else 30.0
            for k in ("loss", "kd", "task"):
                np.testing.assert_allclose(r[k].item(), g[p + k], rtol=1e-5 * f, err_msg=p + k)
            np.testing.assert_allclose(r["w"].cpu().numpy(), g[p + "w"], rtol=2.3e-4 * f, err_msg=p)
            np.testing.assert_allclose(r["gnorm"].item(), g[p + "gnorm"], rtol=(2e-4 if s == 1 else 1e-2), err_msg=p)
            if s == 1:
                ref = g[p + "est"]
                np.testing.assert_allclose(r["est"].cpu().numpy(), ref, rtol=1e-4, atol=1e-4 * float(np.abs(ref).max()))
                coef = min(1.0, 5.0 / (float(g[p + "gnorm"]) + 1e-6))
                bad = []
                for (name, prm), ref_n in zip(model.named_parameters(), g[p + "grad_norm"]):
                    got = float(prm.grad.double().norm())
                    if ref_n < 0:
                        assert got == 0.0, name
                    elif abs(got - ref_n / coef) > (1e-2 if prm.numel() == 1 else 3e-3) * (ref_n / coef) + 1e-6:
                        bad.append((name, got, ref_n / coef))
                assert not bad, bad[:5]
        else:
            assert abs(r["loss"].item() - float(g[p + "loss"])) <= 3.0, (s, r["loss"].item(), float(g[p + "loss"]))


# ------------------------------------------------------------------------------------------------ first layers of row a15
class Cross(nn.Module):
    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, q, k):
        return self.m(q, k, k)[0]


def _hd_layer(name, sd):
    from fqss_amd.quantization.qat import qat_layers as QL
    shp = lambda k: tuple(sd[k].shape)
    if name in ("linearnlq_gelu", "linearnlq_relu"):
        co, ci = shp("linear.weight")
        return QL.LinearNlQ(nn.Linear(ci, co), nn.GELU() if name.endswith("gelu") else nn.ReLU(), **P)
    if name == "nlq_gelu":
        return QL.NlQ(nn.GELU(), **A)
    if name == "conv1dnlq_glu":
        co, ci, _ = shp("conv1d.weight")
        return QL.Conv1dNlQ(nn.Conv1d(ci, co, 1), nn.GLU(dim=1), **P)
    if name == "divq":
        return QL.DivQ(QL.Div(), **A)
    if name == "conv1dq_k3_d2":
        co, ci, k = shp("conv1d.weight")
        return QL.Conv1dQ(nn.Conv1d(ci, co, k, dilation=2, padding=2), **P)
    if name == "conv1dnlq_k8_s4_gelu":
        co, ci, k = shp("conv1d.weight")
        return QL.Conv1dNlQ(nn.Conv1d(ci, co, k, stride=4, padding=2), nn.GELU(), **P)
    if name in ("conv1dgnnlq_gelu", "conv1dgnnlq_glu"):
        co, ci, k = shp("conv1d.weight")
        return QL.Conv1dGnNlQ(nn.Conv1d(ci, co, k, padding=k // 2), nn.GroupNorm(1, co), nn.GELU() if name.endswith("gelu") else nn.GLU(1), **P)
    if name == "conv2dnlq_k8_s4_gelu":
        co, ci = shp("conv2d.weight")[:2]
        return QL.Conv2dNlQ(nn.Conv2d(ci, co, (8, 1), (4, 1), (2, 0)), nn.GELU(), **P)
    if name in ("conv2dnlq_3x3_glu", "conv2dnlq_1x1_glu"):
        co, ci, k, _ = shp("conv2d.weight")
        return QL.Conv2dNlQ(nn.Conv2d(ci, co, k, 1, k // 2), nn.GLU(1), **P)
    if name == "convtr2dnlq_k8_s4_gelu":
        ci, co = shp("convTr2d.weight")[:2]
        return QL.ConvTranspose2dNlQ(nn.ConvTranspose2d(ci, co, (8, 1), (4, 1)), nn.GELU(), **P)
    if name == "convtr1dnlq_k8_s4_gelu":
        ci, co = shp("convTr1d.weight")[:2]
        return QL.ConvTranspose1dNlQ(nn.ConvTranspose1d(ci, co, 8, 4), nn.GELU(), **P)
    if name == "convtr1dq_k5_s3_p1":
        ci, co = shp("convTr1d.weight")[:2]
        return QL.ConvTranspose1dQ(nn.ConvTranspose1d(ci, co, 5, 3, padding=1, output_padding=2), **P)
    if name in ("mhaq_bf_self", "mhaq_bf_cross"):
        e = shp("m.mha.out_proj.weight")[0]
        m = QL.MultiheadAttentionQ(nn.MultiheadAttention(e, 4, dropout=0.0, batch_first=True), **P)
        return First(m, 3) if name.endswith("self") else Cross(m)
    if name == "conv1dencoderq_k8_s4_gelu":
        co, ci, k = shp("conv1d.weight")
        return QL.Conv1dEncoderQ(nn.Sequential(nn.Conv1d(ci // 2, co, k, 4, 2), nn.GELU()), n_splitter=2, **P)
    if name == "conv2dencoderq_k8_s4_gelu":
        co, ci = shp("conv2d.weight")[:2]
        return QL.Conv2dEncoderQ(nn.Sequential(nn.Conv2d(ci // 2, co, (8, 1), (4, 1), (2, 0)), nn.GELU()), n_splitter=2, **P)
    if name == "convtr1ddecoderq_stereo":
        ci, co = shp("convTr1d.weight")[:2]
        return QL.ConvTr1dDecoderQ(nn.Sequential(nn.ConvTranspose1d(ci, co, 8, 4)), n_combiner=2, **P)
    if name == "convtr2ddecoderq_resdec":
        ci, co = shp("convTr2d.weight")[:2]
        return QL.ConvTr2dDecoderQ(nn.Sequential(nn.ConvTranspose2d(ci, co, (8, 1), (4, 1))), n_combiner=2, train_res_dec=True, **P)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["mhaq_bf_self", "mhaq_bf_cross", "conv1dencoderq_k8_s4_gelu", "conv2dencoderq_k8_s4_gelu", "convtr1ddecoderq_stereo", "convtr2ddecoderq_resdec",
                                  "linearnlq_gelu", "linearnlq_relu", "nlq_gelu", "conv1dnlq_glu", "divq", "conv1dq_k3_d2",
                                  "conv1dnlq_k8_s4_gelu", "conv1dgnnlq_gelu", "conv1dgnnlq_glu", "conv2dnlq_k8_s4_gelu",
                                  "conv2dnlq_3x3_glu", "conv2dnlq_1x1_glu", "convtr2dnlq_k8_s4_gelu", "convtr1dnlq_k8_s4_gelu",
                                  "convtr1dq_k5_s3_p1"])
def test_htdemucs_first_layers_teacher_forced(golden, name):
    """SURVEY §8 row a15, layer level (the model is not built yet): GELU / GLU maps, LinearNlQ, DivQ against the reference"""
    g = golden("hd_layers")
    sd = {k[len(name) + 4:]: T(g[k]) for k in g.files if k.startswith(name + ".sd.")}
    L = _hd_layer(name, sd)
    L.load_state_dict(sd, strict=True)
    L = L.cuda().train()
    _leave_observer(L)
    ins, i = [], 0
    while f"{name}.in{i}" in g.files:
        ins.append(T(g[f"{name}.in{i}"]).cuda().requires_grad_(True))
        i += 1
    y = L(*ins)
    y.backward(T(g[f"{name}.gout"]).cuda())
    nflip = 0
    halves = [("activation_fake_quantize", slice(None))]
    if "decoderq" in name:          # stacked (MSB, LSB) outputs, each behind its own quantizer
        halves = [("activation_fake_quantize", 0), ("activation_fake_quantize_residual", 1)]
    if name.startswith("mhaq"):
        halves = [("m.activation_fake_quantize", slice(None))]
    for qn, sel in halves:
        lo, hi = float(sd[qn + ".min_range"]), float(sd[qn + ".max_range"])
        delta = (hi - lo) / 255.0
        a, b = np.rint((y.detach().cpu().numpy()[sel] - lo) / delta), np.rint((g[f"{name}.out"][sel] - lo) / delta)
        assert np.abs(a - b).max() <= 1 and float(np.mean(a != b)) <= 3e-3, (name, qn)
        nflip += int((a != b).sum())
    for i, x in enumerate(ins):
        want = g[f"{name}.gin{i}"]
        bad = np.abs(x.grad.cpu().numpy() - want) > 2e-4 * np.abs(want).max() + 2e-4 * np.abs(want)
        assert bad.mean() <= 2e-3 + 8.0 * nflip / want.size, (name, i, bad.mean())
    params = dict(L.named_parameters())
    for k in g.files:
        if k.startswith(name + ".grad.") and not k.endswith(".decoder_bias"):        # (an alias of the decoder's bias)
            w = g[k]
            np.testing.assert_allclose(params[k[len(name) + 6:]].grad.cpu().numpy(), w, rtol=3e-3, atol=(3e-3 + 0.05 * nflip) * (np.abs(w).max() + 1e-6), err_msg=k)


def test_htdemucs_embeddingq(golden):
    from fqss_amd.quantization.qat import qat_layers as QL
    g = golden("hd_layers")
    sd = {k[len("embeddingq.sd."):]: T(g[k]) for k in g.files if k.startswith("embeddingq.sd.")}
    V, Dm = sd["embedding.weight"].shape
    L = QL.EmbeddingQ(nn.Embedding(V, Dm), **P)
    L.load_state_dict(sd, strict=True)
    L = L.cuda().train()
    _leave_observer(L)
    y = L(T(g["embeddingq.idx"]).cuda())
    y.backward(T(g["embeddingq.gout"]).cuda())
    np.testing.assert_allclose(y.detach().cpu().numpy(), g["embeddingq.out"], rtol=0, atol=1e-6)
    params = dict(L.named_parameters())
    for k in g.files:
        if k.startswith("embeddingq.grad."):
            np.testing.assert_allclose(params[k[len("embeddingq.grad."):]].grad.cpu().numpy(), g[k], rtol=1e-4, atol=1e-6, err_msg=k)


def test_lazy_capture_in_training_loops_matches_eager(golden):
    """trainers call KDTrainStep.maybe_capture(): after the observer phase (and one eager quantizing step) the step is recorded
    WITHOUT being run and replays from then on; a learning-rate change drops the graphs.  Same state in -> same losses out as
    the all-eager twin (up to the fp32 atomics of the weight gradients)"""
    from fqss_amd.runtime import KDTrainStep
    g = golden("dpt_tiny_step")
    x, tgt = T(g["x"]).cuda(), T(g["tgt"]).cuda()
    runs = []
    for lazy in (False, True):
        model, fmodel = _forced(g, 50)
        step = KDTrainStep(model, fmodel, kd_lambda=0.1, lr=4e-4, clip=5.0)
        losses, graphed = [], []
        for i in range(6):
            if lazy:
                step.maybe_capture(x, tgt)
            graphed.append(step._graphs is not None)
            if i == 4:
                step.lr = 2e-4                  # scheduler step
                assert step._graphs is None
                if lazy:
                    step.maybe_capture(x, tgt)
                    assert step._graphs is not None
            losses.append(step(x, tgt)["loss"].item())
        runs.append((losses, graphed, step.arena.flat_p.clone()))
    (l0, g0, p0), (l1, g1, p1) = runs
    assert g0 == [False] * 6 and g1 == [False, True, True, True, True, True]
    np.testing.assert_allclose(l0[0], l1[0], rtol=1e-6)
    np.testing.assert_allclose(l0[1], l1[1], atol=0.05)          # dB: the first replayed step (fp32 atomics of step 1 already differ)
    np.testing.assert_allclose(l0, l1, atol=0.35)                # dB; chaotic after a few quantized updates (0.12 dB seen)
    assert float((p0 - p1).abs().max()) < 5e-3


@pytest.mark.parametrize("R,Ci,Co", [(45, 16, 24), (1000, 64, 192), (777, 256, 1024), (8500, 1024, 256), (130, 64, 512)])
def test_qrow_kernel_exact_integer_sums(R, Ci, Co):
    """the int8-MFMA row q-GEMM: z = dw (dx S + min_x R) + b with S an exact integer, against the same formula in fp64"""
    from fqss_amd import kernels as K
    w = rnd(Co, Ci, seed=51, scale=0.2).cuda()
    lo_w, hi_w = (-(w.abs().amax(1, keepdim=True)) * 0.9), (w.abs().amax(1, keepdim=True) * 0.95)
    wc = K.wq_codes(w, lo_w.contiguous(), hi_w.contiguous())
    xc = torch.randint(0, 256, (R, Ci), generator=torch.Generator().manual_seed(52), dtype=torch.uint8).cuda()
    lo, hi = torch.tensor([-1.3], device="cuda"), torch.tensor([2.1], device="cuda")
    b = rnd(Co, seed=53).cuda()
    z = K.qrow_fwd(xc, wc, b, lo, hi)
    S = xc.cpu().double() @ wc.idx.cpu().double().T
    dx = (hi.cpu() - lo.cpu()) / 255.0
    ref = wc.dw.cpu().double() * (dx.double() * S + lo.cpu().double() * wc.rw.cpu().double()) + b.cpu().double()
    close(z, ref, 2e-6)
    assert torch.equal(wc.rw.cpu(), wc.idx.cpu().float().sum(1))
    # and it agrees with the fp32-equivalent GEMM on the de-quantised operands
    x = dx.cuda() * xc.float() + lo
    wq = wc.dw[:, None] * wc.idx.float()
    close(z, K.rowlin_fwd(x, wq.contiguous(), b), 2e-5)
    # the output quantizer in the GEMM epilogue (fqss_qrow_fwdq) = fqss_qrow_fwd + fqss_actq_fwd, bit for bit
    from fqss_amd import ops
    qlo, qhi, slope = torch.tensor([-0.7], device="cuda"), torch.tensor([1.9], device="cuda"), torch.tensor([0.2], device="cuda")
    for act, sl in ((ops.ACT_NONE, None), (ops.ACT_RELU, None), (ops.ACT_PRELU, slope)):
        z2, y2 = K.qrow_fwdq(xc, wc, b, lo, hi, act, sl, qlo, qhi)
        assert torch.equal(z2, z)
        assert torch.equal(y2, K.actq_fwd(z, act, sl, ops.Q_QUANT, qlo, qhi, None)), act
    # two quantizers and a ReLU in the epilogue (fqss_qrow_fwdq2: LinearQ -> NlQ(ReLU)) = the chain of the three passes, bit for bit
    if Co % 4 == 0:
        q2lo, q2hi = torch.tensor([-0.1], device="cuda"), torch.tensor([1.5], device="cuda")
        z3, y3, c3 = K.qrow_fwdq2(xc, wc, b, lo, hi, qlo, qhi, q2lo, q2hi)
        y1 = K.actq_fwd(z, ops.ACT_NONE, None, ops.Q_QUANT, qlo, qhi, None)
        want = K.actq_fwd(y1, ops.ACT_RELU, None, ops.Q_QUANT, q2lo, q2hi, None)
        assert torch.equal(z3, z) and torch.equal(y3, want)
        d2 = (q2hi - q2lo) / 255.0
        assert torch.equal(c3.float(), torch.round((want - q2lo) / d2).clamp(0, 255))


@pytest.mark.parametrize("R,Ci,Co", [(3000, 64, 512), (129, 16, 8)])
def test_qrow_bwd_w_pair_is_two_coded_weight_gradients(R, Ci, Co, monkeypatch):
    """both directions' W_ih gradients of LSTMQ on the input's codes (two column blocks of dG, one launch) == two launches == fp64"""
    from fqss_amd import kernels as K
    dG = rnd(R, 2 * Co, seed=61).cuda()
    xc = torch.randint(0, 256, (R, Ci), generator=torch.Generator().manual_seed(62), dtype=torch.uint8).cuda()
    lo, hi = torch.tensor([-0.8], device="cuda"), torch.tensor([1.7], device="cuda")
    x = ((hi - lo) / 255.0).double().cpu() * xc.cpu().double() + lo.double().cpu()
    want = [dG[:, :Co].cpu().double().T @ x, dG[:, Co:].cpu().double().T @ x]
    for on in (True, False):
        monkeypatch.setattr(K, "PAIR_WGRAD", on)
        flat = torch.zeros(2 * Co * Ci + 64, device="cuda")
        g0, g1 = flat[:Co * Ci].view(Co, Ci), flat[Co * Ci + 64:].view(Co, Ci)
        K.qrow_bwd_w_pair(dG[:, :Co], dG[:, Co:], xc, lo, hi, g0, g1)
        close(g0, want[0], 1e-5, msg=f"forward direction, pair={on}")
        close(g1, want[1], 1e-5, msg=f"reverse direction, pair={on}")
        assert float(flat[Co * Ci:Co * Ci + 64].abs().max()) == 0


@pytest.mark.parametrize("R,C", [(48500, 64), (1000, 256), (77, 16)])
def test_addq_layernormq_fused_matches_the_two_modules(R, C, monkeypatch):
    """B2-style gate: norm(add(a, b)) with AddQ + LayerNormQ in their quantizing phase as ONE kernel each way (fqss_addq_layernorm_fwd /
    _bwd: the quantized add inside the LayerNorm kernels) against the two modules run one after the other: output bit-identical,
    the gradients of both addends, of gamma / beta and of the four range parameters within fp32 summation noise"""
    from fqss_amd.quantization.qat import qat_layers as QL
    a0, b0, g0 = rnd(R, 1, C, seed=1).cuda(), rnd(R, 1, C, seed=2, scale=0.7).cuda(), rnd(R, 1, C, seed=3).cuda()
    res = {}
    for kind in ("fused", "unfused"):
        monkeypatch.setattr(QL, "FUSE_ADDLN", kind == "fused")
        torch.manual_seed(3)
        add, ln = QL.AddQ(QL.Add(), **{k: v for k, v in A.items() if k != "weight_quant"}).cuda(), QL.LayerNormQ(nn.LayerNorm(C), **A).cuda()
        with torch.no_grad():
            ln.layernorm.weight.copy_(rnd(C, seed=4).cuda() * 0.3 + 1.0)
            ln.layernorm.bias.copy_(rnd(C, seed=5).cuda() * 0.1)
            for _ in range(50):
                ln(add(a0, b0))
        a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        y = QL.addq_layernorm(add, ln, a, b)
        y.backward(g0)
        res[kind] = (y.detach(), a.grad, b.grad, ln.layernorm.weight.grad, ln.layernorm.bias.grad,
                     add.activation_fake_quantize.min_range.grad, add.activation_fake_quantize.max_range.grad,
                     ln.activation_fake_quantize.min_range.grad, ln.activation_fake_quantize.max_range.grad)
        monkeypatch.undo()
    f, u = res["fused"], res["unfused"]
    assert torch.equal(f[0], u[0])
    for i, name in enumerate(("da", "db", "dgamma", "dbeta", "add min", "add max", "ln min", "ln max"), start=1):
        assert f[i] is not None and u[i] is not None, name
        err = float((f[i] - u[i]).norm() / (u[i].norm() + 1e-12))
        assert err <= 2e-5, (name, err)
    assert torch.equal(f[1], f[2])


@pytest.mark.parametrize("to,n0,B,m,C", [("cols", 250, 1, 194, 64), ("rows", 194, 1, 250, 64), ("cols", 10, 2, 7, 16)])
def test_layout_change_inside_the_addq_layernormq_kernels(to, n0, B, m, C, monkeypatch):
    """the intra- <-> inter-chunk layout change behind a DPTNet layer (rows_to_cols / cols_to_rows, dptnetq.py:313-327) done by the fused
    AddQ + LayerNormQ kernels through their row map (fqss_addq_layernorm_fwd_map / _bwd_map) against the same kernels followed by the
    transposing copy: output, the codes that travel with it and every gradient BIT-identical (the arithmetic per row is unchanged)"""
    from fqss_amd.quantization.qat import qat_layers as QL
    a0, b0 = rnd(n0, B * m, C, seed=1).cuda(), rnd(n0, B * m, C, seed=2, scale=0.7).cuda()
    g0 = rnd(m, B * n0, C, seed=3).cuda()
    res = {}
    for kind in ("fused", "copy"):
        monkeypatch.setattr(QL, "FUSE_LN_LAYOUT", kind == "fused")
        torch.manual_seed(3)
        add, ln = QL.AddQ(QL.Add(), **{k: v for k, v in A.items() if k != "weight_quant"}).cuda(), QL.LayerNormQ(nn.LayerNorm(C), **A).cuda()
        with torch.no_grad():
            ln.layernorm.weight.copy_(rnd(C, seed=4).cuda() * 0.3 + 1.0)
            ln.layernorm.bias.copy_(rnd(C, seed=5).cuda() * 0.1)
            for _ in range(50):
                ln(add(a0, b0))
        a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        y = QL.addq_layernorm(add, ln, a, b, (to, B))
        assert tuple(y.shape) == (m, B * n0, C)
        codes = getattr(y, "_fqss_rowq", None)
        assert codes is not None and tuple(codes.idx.shape) == tuple(y.shape)
        y.backward(g0)
        res[kind] = (y.detach(), codes.idx.clone(), a.grad, b.grad, ln.layernorm.weight.grad, ln.layernorm.bias.grad,
                     add.activation_fake_quantize.min_range.grad, add.activation_fake_quantize.max_range.grad,
                     ln.activation_fake_quantize.min_range.grad, ln.activation_fake_quantize.max_range.grad)
        monkeypatch.undo()
    # and the map is the layout change: y[i2][b * n0 + i0] = LN row (i0, b, i2)
    lo, hi = float(res["fused"][0].min()), float(res["fused"][0].max())
    assert hi > lo
    for i, (f, u) in enumerate(zip(res["fused"], res["copy"])):
        assert f is not None and u is not None, i
        if i < 4:
            assert torch.equal(f, u), i
        else:       # column / range sums: the same terms, grouped by workgroup in another row order
            assert float((f - u).norm() / (u.norm() + 1e-12)) <= 2e-5, i


def test_coded_row_linear_gradients_do_not_read_carriers(monkeypatch):
    """regression: under the codes-only dataflow of KDTrainStep (ops.fast_codes) a row quantizer feeding a linear on codes must still
    write its fp32 values -- the linear's weight gradient reads them.  Carriers are NaN-poisoned here (ops.DEBUG_POISON)."""
    from fqss_amd import ops
    from fqss_amd.quantization.qat import qat_layers as QL
    monkeypatch.setattr(ops, "DEBUG_POISON", True)
    torch.manual_seed(0)
    ln = QL.LayerNormQ(nn.LayerNorm(64), **A).cuda()
    lin = QL.LinearQ(nn.Linear(64, 32), **P).cuda()
    x = torch.randn(6, 20, 64, device="cuda")
    with torch.no_grad():
        for _ in range(50):
            lin(ln(x))
    grads = []
    for fast in (False, True):
        for p in list(ln.parameters()) + list(lin.parameters()):
            p.grad = None
        xi = x.clone().requires_grad_(True)
        with ops.fast_codes(fast):
            y = lin(ln(xi))
        y.backward(torch.ones_like(y))
        assert torch.isfinite(lin.linear.weight.grad).all() and torch.isfinite(xi.grad).all()
        grads.append((lin.linear.weight.grad.clone(), xi.grad.clone()))
    np.testing.assert_allclose(grads[0][0].cpu().numpy(), grads[1][0].cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(grads[0][1].cpu().numpy(), grads[1][1].cpu().numpy(), rtol=1e-5, atol=1e-6)


def test_dptnet_backward_segments_match_the_single_pass_backward():
    """gradient buckets for cfg 3 (DPTNetQ.fqss_segments): the full-size network's backward as 3 segments of two (row, col) transformer
    pairs each, the encoder -> mask-multiply edge as a late cut, against the one-pass backward"""
    from tests.helpers_segments import check_backward_segments
    x, tgt = O.synth_batch(1, 8000, seed=4)
    check_backward_segments(lambda: build_pair(2), x.cuda(), tgt.cuda(), nb=3, nseg=3)


@pytest.mark.parametrize("C", [64, 256, 384])
def test_layernormq_one_kernel_each_way_equals_the_two_node_form(C, monkeypatch):
    """LayerNormQ in the quantizing phase: LayerNorm + output quantizer as ONE kernel each way (ops_dp.LayerNormRowsQ,
    fqss_layernormq_fwd/bwd) against the separate fqss_layernorm_* + fqss_actq_* launches -- same arithmetic, so the output, its codes
    and dL/dx are bit-identical; the affine and range gradients differ by summation order only"""
    from fqss_amd import ops
    from fqss_amd.quantization.qat import qat_layers as QL
    res = []
    x0 = rnd(37, 11, C, seed=5, scale=1.3)
    g0 = rnd(37, 11, C, seed=6)
    for fuse in (False, True):
        monkeypatch.setattr(QL, "FUSE_LNQ", fuse)
        torch.manual_seed(0)
        ln = nn.LayerNorm(C)
        with torch.no_grad():
            ln.weight.copy_(rnd(C, seed=7, scale=0.3) + 1.0)
            ln.bias.copy_(rnd(C, seed=8, scale=0.2))
        L = QL.LayerNormQ(ln).cuda()
        aq = L.activation_fake_quantize
        aq.n_iter = aq.max_observations
        with torch.no_grad():
            aq.min_range.fill_(-1.1)          # clips a few percent of the values on both sides
            aq.max_range.fill_(1.4)
        x = x0.cuda().requires_grad_(True)
        with ops.coded_dataflow(True):
            y = L(x)
        codes = getattr(y, "_fqss_rowq", None)
        y.backward(g0.cuda())
        res.append((y.detach(), codes.idx.clone() if codes is not None else None, x.grad.clone(), ln.weight.grad.clone(), ln.bias.grad.clone(),
                    aq.min_range.grad.clone(), aq.max_range.grad.clone()))
    (y0, c0, gx0, gg0, gb0, gmn0, gmx0), (y1, c1, gx1, gg1, gb1, gmn1, gmx1) = res
    assert torch.equal(y0, y1) and torch.equal(gx0, gx1)
    assert c0 is not None and c1 is not None and torch.equal(c0, c1)
    frac = float(((c1 == 0) | (c1 == 255)).float().mean())
    assert 0.01 < frac < 0.6, frac
    close(gg1, gg0, 1e-5)
    close(gb1, gb0, 1e-5)
    close(gmn1, gmn0, 1e-5)
    close(gmx1, gmx0, 1e-5)


@pytest.mark.parametrize("Ci,Co,relu", [(64, 256, True), (256, 64, False), (64, 1024, True), (96, 200, False)])
def test_linearq_one_node_equals_the_separate_nodes(Ci, Co, relu, monkeypatch):
    """LinearQ / LinearNlQ in the quantizing phase as ONE autograd node whose quantizer backward also sums the bias gradient
    (ops_dp.RowLinearActQ, fqss_actq_bwd_colbias) against row linear + quantizer node + fqss_colsum: output and dL/dx bit-identical,
    bias / weight / range gradients equal up to summation order.  (200 features: the last 64-feature slice of the kernel is partial.)"""
    from fqss_amd.quantization.qat import qat_layers as QL
    res = []
    x0 = rnd(50, 20, Ci, seed=5, scale=1.0)
    g0 = rnd(50, 20, Co, seed=6)
    for fuse in (False, True):
        monkeypatch.setattr(QL, "FUSE_ROWQ", fuse)
        torch.manual_seed(0)
        lin = nn.Linear(Ci, Co)
        with torch.no_grad():
            lin.bias.copy_(rnd(Co, seed=8, scale=0.2))
        L = (QL.LinearNlQ(lin, nn.ReLU()) if relu else QL.LinearQ(lin)).cuda()
        x = x0.cuda().requires_grad_(True)
        with torch.no_grad():
            L(x)                                   # observer call: weight ranges recorded, activation range from the data
        aq = L.activation_fake_quantize
        aq.n_iter = aq.max_observations
        with torch.no_grad():
            aq.min_range.fill_(-0.2 if relu else -0.9)
            aq.max_range.fill_(1.1)
        y = L(x)
        y.backward(g0.cuda())
        res.append((y.detach(), x.grad.clone(), lin.bias.grad.clone(), lin.weight.grad.clone(), aq.min_range.grad.clone(),
                    aq.max_range.grad.clone()))
    (y0, gx0, gb0, gw0, gmn0, gmx0), (y1, gx1, gb1, gw1, gmn1, gmx1) = res
    assert torch.equal(y0, y1) and torch.equal(gx0, gx1)
    assert float(gb0.abs().max()) > 0
    close(gb1, gb0, 1e-5)
    close(gw1, gw0, 1e-5)
    close(gmn1, gmn0, 1e-5)
    close(gmx1, gmx0, 1e-5)


def test_dptnet_batched_quantizer_tables_cover_every_weight():
    """QuantTables on the tiny DPTNet: all 36 weight quantizers (convolutions, LinearQ, attention projections, the four LSTM matrices
    of every LSTMQ, the 1x1 Conv2dQ, the linear decoder) run from the tables -- output bit-identical, every gradient equal"""
    from tests.helpers_segments import check_batched_tables
    x, tgt = O.synth_batch(1, 4000, seed=3)
    check_batched_tables(lambda: build_pair(0, **TINY), x.cuda(), tgt.cuda(), 36, step_kw=dict(kd_lambda=0.1, clip=0.0))


@pytest.mark.parametrize("R,Ci,Co", [(8500, 256, 1024), (8500, 1024, 256), (4850, 64, 256), (777, 64, 192), (300, 256, 768)])
def test_coded_gradient_row_gemms(R, Ci, Co):
    """fqss_qrow_bwd_x / fqss_qrow_bwd_w (the student's row-major dgrad / wgrad on the 8-bit codes: one exact bf16 plane, three products
    per k) against fp64 and against the fp32 x fp32 form on the de-quantized operands: same fp32-grade accuracy"""
    from fqss_amd import kernels as K
    torch.manual_seed(R + Ci)
    dev = "cuda"
    gz = torch.randn(R, Co, device=dev) * torch.exp(torch.randn(R, Co, device=dev)) * 1e-3
    w = torch.randn(Co, Ci, device=dev) * 0.05
    rng = torch.full((Co, 1), 0.17, device=dev)
    wc = K.wq_codes(w, -rng, rng)
    wq = (wc.idx.float() * wc.dw[:, None]).contiguous()                       # the fake-quantized weight, exactly
    xc = torch.randint(0, 256, (R, Ci), device=dev, dtype=torch.uint8)
    lo, hi = torch.tensor([-1.3], device=dev), torch.tensor([2.1], device=dev)
    x = (xc.float() * ((hi - lo) / 255.0) + lo).contiguous()
    # dgrad
    gx = K.qrow_bwd_x(gz, wc)
    gx_f = K.rowlin_bwd_x(gz, wq)
    ref = gz.double() @ wq.double()
    nrm = float(ref.norm())
    assert float((gx.double() - ref).norm()) <= 1e-6 * nrm and float((gx_f.double() - ref).norm()) <= 1e-6 * nrm
    assert float((gx - gx_f).abs().max()) <= 2e-6 * float(ref.abs().max())
    # wgrad (accumulating)
    gw = torch.full((Co, Ci), 0.5, device=dev)
    K.qrow_bwd_w(gz, xc, lo, hi, gw)
    gw_f = torch.full((Co, Ci), 0.5, device=dev)
    K.rowlin_bwd_w(gz, x, gw_f)
    ref = 0.5 + gz.double().t() @ (xc.double() * ((hi - lo).double() / 255.0) + lo.double())
    nrm = float((ref - 0.5).norm())
    assert float((gw.double() - ref).norm()) <= 2e-6 * nrm, float((gw.double() - ref).norm()) / nrm
    assert float((gw_f.double() - ref).norm()) <= 2e-6 * nrm
    # the same launch with the bias gradient on the side (fqss_qrow_bwd_wb): gw unchanged, gbias += column sums of gz
    gw_b, gb = torch.full((Co, Ci), 0.5, device=dev), torch.full((Co,), 0.25, device=dev)
    K.qrow_bwd_w(gz, xc, lo, hi, gw_b, gb)
    assert float((gw_b.double() - ref).norm()) <= 2e-6 * nrm
    close(gb, 0.25 + gz.double().sum(0), 5e-6)
