"""The residual AddQ's backward in the epilogue of the dgrad that produces its gradient (csrc/qgemm.hip k_qgemm<1, 3, false, true>,
fqss_qpw_bwd_x_addq + fqss_bias_ws_reduce; ops.FUSE_ADD_DGRAD).

1. At the C ABI against the two-launch path it replaces -- fqss_qpw_bwd_x_add, then fqss_ewq_bwd_p with the producer of operand b fused --
   on guarded, NaN-filled buffers with a different row pitch per tensor: dL/da and the producer's gz are torch.equal (both kernels call
   ONE per-element function, csrc/fqss_dev.h), the row padding is left as that path leaves it.  The range partials of both quantizers
   and the producer's bias gradient are sums in another order, so they are compared with a float64 reference computed on the CPU from
   the same operands (the quantizer decisions in the kernels' own fp32 operation sequence): the bound is 4 x the error of the
   two-launch path against that reference on the same case (both form fp32 partial sums per thread and finish in fp64; the fused
   form's per-thread sums are shorter), and three wrong kernels -- the fork's addend dropped, the producer's range swapped with the
   add's, the bias sum stored in the neighbouring row's slot -- must exceed it.
2. Refusals leave the outputs untouched.  3. The bias gradient has the same bits run after run (no float atomics).
4. The training step takes the path (tiny ConvTasNet): five launches of the AddQ backward fewer, same estimates, loss and gradients,
   eagerly and as a hipGraph replay; not across a backward cut; a third consumer of the declared tensor raises.

Measured on the MI355X (e = |got - ref| / |ref| over the four range partials / the bias vector; two-launch path | fused; with addend):
    (1, 128, 16, 1)     partials 6.38e-08 | 8.87e-08    bias 3.48e-08 | 3.48e-08
    (2, 128, 64, 65)    partials 1.97e-07 | 3.32e-07    bias 8.93e-08 | 7.77e-08
    (3, 48, 32, 63)     partials 7.80e-08 | 1.76e-07    bias 8.61e-08 | 6.88e-08
    (1, 128, 512, 130)  partials 9.97e-08 | 1.04e-07    bias 9.20e-08 | 8.88e-08
    (2, 16, 16, 64)     partials 6.70e-08 | 8.03e-08    bias 7.89e-08 | 1.15e-07
every mutation floor 0.3 .. 2.6 (profiles/r07_addq_dgrad_isolated.txt)
"""
import types

import pytest
import torch

import tests.test_gpu_qgemm_kernels as Q
from tests.test_gpu_layout_spectral_kernels import F64, Blk, Vec, all_unchanged, gpu, refused, stream
from tests.test_gpu_qgemm_kernels import _gpu  # noqa: F401  (the fixture behind @gpu: binds the library for the helpers)

CASES = [(1, 128, 16, 1), (2, 128, 64, 65), (3, 48, 32, 63), (1, 128, 512, 130), (2, 16, 16, 64)]   # (B, Ci, Co, M)
RA, RB, RY = (-1.0, 1.2), (-0.8, 0.9), (-1.1, 1.3)        # ranges of the add's operands a, b (= the producer's quantizer) and of its own
SLOTS3 = 2048 * 3


def operands(B, Ci, Co, M, seed, addend=True):
    g = Q.gen(seed)
    o = _operands(g, B, Ci, Co, M)
    if not addend:
        o["add"] = None
    return o


def _operands(g, B, Ci, Co, M):
    return dict(wi=Q.wcodes(g, Co, Ci), dw=Q.steps(g, Co), gz=Q.heavy(g, B, Co, M), add=Q.heavy(g, B, Ci, M, scale=3e-2),
                a=Q.codes(g, B, Ci, M), b=Q.codes(g, B, Ci, M), pz=torch.randn(B, Ci, M, generator=g) * 0.7)


def q32(t, r):
    """(in range, clamped code, pre-round coordinate) of the kernels' fq_asym, in their fp32 operation sequence"""
    lo, d = Q.f32(r[0]), Q.delta32(*r)
    u = (t.float() - lo) / d
    X = torch.round(u)
    return (X >= 0) & (X <= 255), X.clamp(0, 255).double(), u.double()


def dec32(c, r):
    return Q.delta32(*r) * c.float() + Q.f32(r[0])


def reference(o, drop_addend=False, swap=False, roll=False):
    """float64: (the four range partials [add dmin, add dmax, producer dmin, producer dmax], the producer's bias gradient [Ci]) and the
    in-range masks of both quantizers"""
    g = Q.dgrad_ref(o["wi"], o["dw"], o["gz"], None if (drop_addend or o["add"] is None) else o["add"])
    ry, rb = (RB, RY) if swap else (RY, RB)
    z = dec32(o["a"], RA) + dec32(o["b"], RB)
    inr, cq, u = q32(z, ry)
    du, po = (g * torch.where(inr, cq - u, cq)).sum(), (g * (~inr).double()).sum()
    gt = g * inr.double()
    pin, pc, pu = q32(o["pz"], rb)
    bdu, bpo = (gt * torch.where(pin, pc - pu, pc)).sum(), (gt * (~pin).double()).sum()
    bias = (gt * pin.double()).sum((0, 2))
    if roll:
        bias = bias.roll(1)
    part = torch.stack([po - du / 255.0, du / 255.0, bpo - bdu / 255.0, bdu / 255.0])
    return part, bias, inr, pin


class Run:
    """both paths on guarded buffers; every tensor with its own row pitch"""

    def __init__(self, B, Ci, Co, M, o):
        r4, r16 = Q.r4, Q.r16
        self.dims = (B, Ci, Co, M)
        self.gz = Blk(B * Co, M, r4(M) + 4, fill=o["gz"])
        self.add = Blk(B * Ci, M, r4(M) + 8, fill=o["add"]) if o["add"] is not None else None
        self.addp, self.addld = (self.add.ptr, self.add.ld) if self.add is not None else (None, 0)
        self.wT, self.dw = Q.Cod(Ci, Co, fill=o["wi"].t()), Vec(Co, fill=o["dw"])
        self.a, self.b = Q.Cod(B * Ci, M, r16(M) + 16, fill=o["a"]), Q.Cod(B * Ci, M, r16(M) + 32, fill=o["b"])
        self.pz = Blk(B * Ci, M, r4(M) + 12, fill=o["pz"])
        self.pz.padv[:, :r4(M) - M] = 0.25        # z's row padding up to a multiple of 4 is finite in real use: the forward GEMM writes it
        self.pz.before = self.pz.buf.clone()
        self.r = [Q.sc(v) for v in RA + RB + RY]
        self.ops = dict(gz=self.gz, wT=self.wT, **({"add": self.add} if self.add is not None else {}), dw=self.dw, a=self.a, b=self.b, pz=self.pz,
                        **{f"r{i}": v for i, v in enumerate(self.r)})

    def outputs(self):
        B, Ci, Co, M = self.dims
        return (Blk(B * Ci, M, Q.r4(M) + 16), Blk(B * Ci, M, Q.r4(M) + 20), Vec(SLOTS3, fill=0.0, dtype=F64), Vec(SLOTS3, fill=0.0, dtype=F64),
                Vec(Ci, fill=0.0))

    def two_launch(self):
        B, Ci, Co, M = self.dims
        ga, pout, gacc, pgacc, gbias = self.outputs()
        gx = Blk(B * Ci, M, Q.r4(M) + 24)
        r = self.r
        if self.add is not None:
            Q.call("fqss_qpw_bwd_x_add", self.gz.ptr, self.wT.ptr, self.dw.ptr, self.add.ptr, gx.ptr, B, Ci, Co, M, self.gz.ld, self.add.ld, gx.ld,
                   stream())
        else:
            Q.call("fqss_qpw_bwd_x", self.gz.ptr, self.wT.ptr, self.dw.ptr, gx.ptr, B, Ci, Co, M, self.gz.ld, gx.ld, stream())
        Q.call("fqss_ewq_bwd_p", self.a.ptr, r[0].ptr, r[1].ptr, self.b.ptr, r[2].ptr, r[3].ptr, 1.0, gx.ptr, ga.ptr, B * Ci, M, self.a.ld,
               self.b.ld, gx.ld, ga.ld, Q.ACT_NONE, None, r[4].ptr, r[5].ptr, gacc.ptr, Ci, None, 0, 0, None, None, None, None, 0,
               self.pz.ptr, self.pz.ld, Q.ACT_NONE, None, pgacc.ptr, gbias.ptr, pout.ptr, pout.ld, stream())
        all_unchanged(**self.ops)
        return ga, pout, gacc, pgacc, gbias

    def record(self, o_ga, o_pout, o_gacc, o_pgacc, o_ws, **over):
        r = self.r
        s = Q._lib.FqssAddqBwd()
        s.a, s.ld_a, s.amin, s.amax = self.a.ptr, self.a.ld, r[0].ptr, r[1].ptr
        s.b, s.ld_b, s.bmin, s.bmax = self.b.ptr, self.b.ld, r[2].ptr, r[3].ptr
        s.qmin, s.qmax, s.gacc = r[4].ptr, r[5].ptr, o_gacc.ptr
        s.pz, s.ld_pz, s.pgacc = self.pz.ptr, self.pz.ld, o_pgacc.ptr
        s.pout, s.ld_pout, s.ga, s.ld_ga = o_pout.ptr, o_pout.ld, o_ga.ptr, o_ga.ld
        s.bias_ws, s.bias_ws_floats = o_ws.ptr, o_ws.t.numel()
        for k, v in over.items():
            setattr(s, k, v)
        return s

    def fused(self):
        B, Ci, Co, M = self.dims
        ga, pout, gacc, pgacc, gbias = self.outputs()
        nwg = Q._lib.query("fqss_qpw_bwd_x_addq_wgs", B, M)
        assert nwg == B * ((M + 63) // 64)
        ws = Vec(nwg * Ci)
        s = self.record(ga, pout, gacc, pgacc, ws)
        Q.call("fqss_qpw_bwd_x_addq", self.gz.ptr, self.wT.ptr, self.dw.ptr, self.addp, B, Ci, Co, M, self.gz.ld, self.addld,
               Q.ctypes.byref(s), stream())
        assert ws.written()
        job = Q._lib.FqssBiasWsJob()
        job.ws, job.gbias, job.nwg, job.C = ws.ptr, gbias.ptr, nwg, Ci
        Q.call("fqss_bias_ws_reduce", Q.ctypes.byref(job), 1, stream())
        all_unchanged(**self.ops)
        return ga, pout, gacc, pgacc, gbias


def rel(a, ref):
    return float((a.double().cpu() - ref).norm() / ref.norm())


def partials(gacc, pgacc):
    assert gacc.guards() and pgacc.guards()
    s, p = gacc.t.cpu().view(-1, 3).sum(0), pgacc.t.cpu().view(-1, 3).sum(0)
    assert float(s[2]) == 0.0 and float(p[2]) == 0.0           # no PReLU anywhere: the slope slots stay empty
    return torch.stack([s[0], s[1], p[0], p[1]])


@gpu
@pytest.mark.parametrize("addend", [True, False], ids=["addend", "no-addend"])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_fused_addq_backward_against_the_two_launch_path(case, addend):
    """addend False: the last block of the stack -- the fork's other branch carries no gradient, the two-launch path is fqss_qpw_bwd_x"""
    B, Ci, Co, M = case
    o = operands(B, Ci, Co, M, seed=11 + Co + M, addend=addend)
    part, bias, inr, pin = reference(o)
    for name, m in (("add", inr), ("producer", pin)):
        f = float(m.double().mean())
        assert 0.05 <= f <= 0.95, (name, f)                   # both classes of both quantizers are at least 5 % of the elements
    run = Run(B, Ci, Co, M, o)
    ga2, po2, gacc2, pgacc2, gb2 = run.two_launch()
    ga1, po1, gacc1, pgacc1, gb1 = run.fused()
    for one, two in ((ga1, ga2), (po1, po2)):
        assert Q.fwritten(one) and Q.fwritten(two)
        assert torch.equal(one.view, two.view)
        assert torch.equal(one.padv[:, :Q.r4(M) - M], two.padv[:, :Q.r4(M) - M])      # the row padding as the two-launch path leaves it
    assert gb1.guards() and gb2.guards()
    e2p, e1p = rel(partials(gacc2, pgacc2), part), rel(partials(gacc1, pgacc1), part)
    e2b, e1b = rel(gb2.t, bias), rel(gb1.t, bias)
    bp, bb = 4.0 * e2p, 4.0 * e2b
    print(f"MEAS addq partials two-launch {e2p:.2e} fused {e1p:.2e} bound {bp:.1e} | bias two-launch {e2b:.2e} fused {e1b:.2e} bound {bb:.1e} | {case}"
          f"{'' if addend else ' no addend'}")
    muts = [("producer range swapped with the add's", dict(swap=True), True), ("bias slot of the neighbouring row", dict(roll=True), False)]
    if addend:
        muts.append(("addend dropped", dict(drop_addend=True), True))
    for what, kw, both in muts:
        mp, mb, _, _ = reference(o, **kw)
        fp, fb = rel(mp, part), rel(mb, bias)
        print(f"FLOOR addq {what}: partials {fp:.2e} (bound {bp:.1e}) bias {fb:.2e} (bound {bb:.1e}) | {case}")
        assert fb > bb and (fp > bp or not both), (case, what, fp, bp, fb, bb)
    assert e1p <= bp and e1b <= bb, (case, e1p, bp, e1b, bb)


@gpu
def test_fused_addq_backward_refusals():
    B, Ci, Co, M = 1, 16, 32, 70
    o = operands(B, Ci, Co, M, seed=5)
    run = Run(B, Ci, Co, M, o)
    ga, pout, gacc, pgacc, gbias = run.outputs()
    ws = Vec(2 * Ci)
    wide = Q.Cod(Ci, 1040, fill=torch.zeros(Ci, 1040, dtype=torch.int8))
    dwide = Vec(1040, fill=1.0)
    S = stream()

    def no(msg=None, B=B, Ci=Ci, Co=Co, M=M, wT=run.wT.ptr, dw=run.dw.ptr, add=run.add.ptr, ld_gz=run.gz.ld, ld_add=run.add.ld, rec=True, **over):
        s = run.record(ga, pout, gacc, pgacc, ws, **over)
        m = refused("fqss_qpw_bwd_x_addq", run.gz.ptr, wT, dw, add, B, Ci, Co, M, ld_gz, ld_add, Q.ctypes.byref(s) if rec else None, S,
                    who="qpw_bwd_x")
        assert msg is None or msg in m, m

    no("Ci <= 128", Ci=130)
    no("Co <= 1024", Co=1040, wT=wide.ptr, dw=dwide.ptr)
    no(rec=False)
    for member in ("a", "b", "amin", "amax", "bmin", "bmax", "qmin", "qmax", "gacc", "pz", "pgacc", "pout", "ga", "bias_ws"):
        no(**{member: None})
    no(ld_a=run.a.ld + 4)                    # code rows
    no(a=run.a.ptr + 4)
    no(ld_b=64)
    no(ld_pz=run.pz.ld + 2)                  # fp32 rows
    no(pz=run.pz.ptr + 4)
    no(ld_pout=68)
    no(pout=pout.ptr + 8)
    no(ld_ga=pout.ld + 1)
    no(ga=ga.ptr + 4)
    no(ld_add=run.add.ld + 2)
    no("workspace too small", bias_ws_floats=2 * Ci - 1)
    big = dict(ld_a=4032, ld_b=4032, ld_pz=4032, ld_pout=4032, ld_ga=4032)
    no("slots", B=33, M=4032, ld_gz=4032, ld_add=4032, **big)                # 33 x 63 = 2079 workgroups, 2048 slots; refused before any access
    assert ga.untouched() and pout.untouched() and ws.untouched() and gbias.unchanged() and gacc.unchanged() and pgacc.unchanged()
    all_unchanged(**run.ops)
    job = Q._lib.FqssBiasWsJob()
    job.ws, job.gbias, job.nwg, job.C = ws.ptr, None, 2, Ci
    refused("fqss_bias_ws_reduce", Q.ctypes.byref(job), 1, S)
    refused("fqss_bias_ws_reduce", None, 1, S)
    assert gbias.unchanged()


@gpu
def test_fused_bias_gradient_is_reproducible():
    B, Ci, Co, M = 2, 128, 64, 330
    o = operands(B, Ci, Co, M, seed=21)
    run = Run(B, Ci, Co, M, o)
    first, second = run.fused(), run.fused()
    assert float(first[4].t.abs().max()) > 0
    assert torch.equal(first[4].t, second[4].t)


# ------------------------------------------------------------------------------------------------------------------- 4. the path
TINY = dict(n_spks=2, kernel_size=16, stride=8, n_filters=64, bn_chan=32, hid_chan=64, n_blocks=3, n_repeats=2)


def _steps(monkeypatch, fuse, replay=False, **kw):
    """the tiny ConvTasNet of test_skip_chain_backward_is_taken_and_changes_nothing: third (quantizing) step, carriers poisoned"""
    from fqss_amd import kernels as K
    from fqss_amd import ops
    from fqss_amd.data import synth_batch
    from fqss_amd.quantization.qat import qat_quant as QQ
    from fqss_amd.runtime import KDTrainStep
    from fqss_amd.smoke import build_pair
    x, tgt = synth_batch(2, 4000, seed=3, device="cuda")
    monkeypatch.setattr(ops, "FUSE_ADD_DGRAD", fuse)
    model, fmodel = build_pair("cuda", 0, **TINY)
    step = KDTrainStep(model, fmodel, lr=0.0, **kw)
    step(x, tgt)
    for m in model.modules():
        if isinstance(m, QQ.GradientActivationFakeQuantize):
            m.n_iter = m.max_observations
    step(x, tgt)
    n = {"ewq": 0, "addq": 0}
    real, real_f = K.ewq_bwd_p, K.qpw_bwd_x_addq

    def counted(*a, **k):
        n["ewq"] += 1
        return real(*a, **k)

    def counted_f(*a, **k):
        n["addq"] += 1
        return real_f(*a, **k)
    monkeypatch.setattr(K, "ewq_bwd_p", counted)
    monkeypatch.setattr(K, "qpw_bwd_x_addq", counted_f)
    with ops.poison_carriers(True):
        r = step(x, tgt)
        res = [(r["est"].clone(), r["loss"].item(), step.arena.flat_g.clone())]
        n["eager"] = dict(n)            # the capture pass below keeps counting
        if replay:
            step.capture(x, tgt, warmup=0)
            step.arena.flat_g.fill_(float("nan"))
            r = step(x, tgt)
            res.append((r["est"].clone(), r["loss"].item(), step.arena.flat_g.clone()))
    torch.cuda.synchronize()
    monkeypatch.undo()
    return res, dict(n.pop("eager"), total=n)


def _same(a, b):
    assert torch.equal(a[0], b[0]) and a[1] == b[1]
    assert torch.isfinite(a[2]).all()
    assert float((a[2] - b[2]).norm() / b[2].norm()) <= 1e-6      # float atomics in the other bias gradients: not bit-stable run to run


@pytest.mark.gpu
def test_add_backward_in_the_dgrad_epilogue_is_taken_and_changes_nothing(monkeypatch):
    (on, on_replay), n_on = _steps(monkeypatch, True, replay=True)
    (off,), n_off = _steps(monkeypatch, False)
    # 6 blocks: conv1 of blocks 1..5 takes the residual add of the block in front, in the eager step and in the captured one
    assert n_on["addq"] == 5 and n_off["addq"] == 0 and n_on["total"]["addq"] > 5, (n_on, n_off)      # (> 5: the capture took the path too)
    assert n_off["ewq"] - n_on["ewq"] == 5 and n_on["ewq"] == 0, (n_on, n_off)
    _same(on, off)
    _same(on_replay, off)
    assert torch.equal(on_replay[0], on[0])


@pytest.mark.gpu
def test_add_backward_is_not_fused_across_a_backward_cut(monkeypatch):
    (on,), n_on = _steps(monkeypatch, True, buckets=3)       # cut points after blocks 1 and 3: the links 1 -> 2 and 3 -> 4 are not handed over
    (off,), n_off = _steps(monkeypatch, False, buckets=3)
    assert n_on["addq"] == 3 and n_off["ewq"] - n_on["ewq"] == 3, (n_on, n_off)
    _same(on, off)


def test_a_third_consumer_of_the_declared_tensor_raises():
    """bookkeeping, no device: the conv branch's dgrad consumed the fork's gradient (it ran the backward of the add in front), and the
    other branch turns out to have a consumer whose gradient that dgrad never saw"""
    from fqss_amd import ops
    fk = ops._ForkState()
    other, dummy = torch.zeros(1, 2, 4), torch.empty(1, 2, 4)
    fk.leave(other, 1)
    assert fk.take(0, other.shape) is other
    fk.consumed = dummy
    fk.n_other += 1                           # a further element-wise consumer of branch 1 left its gradient after the conv took its snapshot
    with pytest.raises(RuntimeError, match="declare_add_dgrad"):
        ops.Fork2.backward(types.SimpleNamespace(fk=fk), dummy, torch.zeros(1, 2, 4))
    assert fk.consumed is None and fk.fused_branch is None
    # the add's own node: the gradient it receives must be the placeholder
    link = ops._AddLink(*([None] * 10))
    assert link.pre is None and link.dummy is None and link.fork is None
