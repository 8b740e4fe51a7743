"""GPU: the PIT / KD loss kernels at one and three sources (csrc/train_ops.hip: k_kd_moments_n<S>, k_kd_final_n<S>, k_kd_grad_n behind
fqss_kd_loss_n / fqss_kd_moments_n) against tests/golden/nsrc_loss.npz and the live oracle -- the bodies of tests/nsrc_common.py, which
tests/test_nsrc_cpu.py runs on the CPU backend -- plus what only exists on the device: the S = 2 instantiation held against the
two-source entry points, the refused arguments, the three-source training step eagerly and as a hipGraph replay, the q-GEMM data
gradient above 1024 output channels (the full-size three-source mask conv), and the trainer CLI.

Shapes: T = 1000 (the fixture), 255 / 256 / 257 (around the block width), 16389 (past 64 x 256: the grid-stride loop of the moment
pass takes a second trip); B = 1, 6 and 70 (more than one wave in the one-block kernel; the six-sample pattern repeated)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import fqss_oracle as O
from tests import nsrc_common as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = lambda t: t.cuda()
SHAPES = [(6, 1000), (6, 255), (6, 256), (6, 257), (6, 16389), (1, 1000), (70, 257)]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_three_source_loss_fixture(golden):
    """all six permutations, the two 3-cycles among them (samples 3 and 4): loss, kd, task, w, SI-SDR, dL/d est"""
    from fqss_amd import kernels as K
    N.check_fixture(K, DEV, golden("nsrc_loss"))


@pytest.mark.parametrize("S", [3, 1])
@pytest.mark.parametrize("B,T_", SHAPES)
def test_kd_loss_against_oracle(S, B, T_):
    from fqss_amd import kernels as K
    N.check_kd_loss(K, DEV, S, B, T_)


@pytest.mark.parametrize("S", [3, 1])
@pytest.mark.parametrize("B,T_", SHAPES)
def test_pit_sisdr_against_oracle(S, B, T_):
    from fqss_amd import kernels as K
    N.check_pit_sisdr(K, DEV, S, B, T_)


@pytest.mark.parametrize("S", [3, 1])
@pytest.mark.parametrize("T_", [1000, 255, 256, 257, 16389])
def test_per_sample_objective_against_oracle(S, T_):
    """B = 1 and B = n_src, four thresholds; at S = 3 the batch starts at sample 3, so that both 3-cycles are in"""
    from fqss_amd import kernels as K
    N.check_speechbrain(K, DEV, S, T_, first=3 if S == 3 else 0)


@pytest.mark.parametrize("S", [3, 1])
@pytest.mark.parametrize("B,T_", SHAPES)
def test_moments_against_fp64(S, B, T_):
    from fqss_amd import kernels as K
    N.check_moments(K, DEV, S, B, T_)


def test_evaluation_forms_slice_the_table_by_n_src():
    from fqss_amd.train_env.asteroid_librimix import wsdr
    for S in (3, 1):
        s, e, f = N.batch(S, 6, 1000)
        pw = wsdr.PairwiseWSDR("sisdr", take_log=True)(e.cuda(), s.cuda())
        assert pw.shape == (6, S, S)
        np.testing.assert_allclose(pw.cpu().numpy(), O.pairwise_sisdr(e.double(), s.double(), take_log=True).numpy(), atol=1e-3)
        per = torch.stack([-O.neg_sisdr_pit(e[b:b + 1].double(), s[b:b + 1].double()) for b in range(6)])
        np.testing.assert_allclose(wsdr.si_sdr(e.cuda(), s.cuda()).cpu().numpy(), per.numpy(), atol=1e-3)
        diag = -torch.diagonal(O.pairwise_sisdr(e.double(), s.double()), dim1=1, dim2=2)
        np.testing.assert_allclose(float(wsdr.sisdr(e.cuda(), s.cuda())), float(diag.mean()), rtol=1e-5)


def _loss_n(est, fest, tgt, mode, kd_lambda=0.1, threshold=None):
    """fqss_kd_loss_n called directly (kernels.kd_loss sends S = 2 to the two-source entry points)"""
    from fqss_amd import _lib, kernels as K
    B, S, T_ = est.shape
    dev = est.device
    stats = torch.empty(B, K.KD_STATS_STRIDE_N, device=dev, dtype=torch.float64)
    out, w, sisdr, gest = torch.empty(4, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty_like(est)
    _lib.call("fqss_kd_loss_n", est.data_ptr(), fest.data_ptr(), tgt.data_ptr(), B, S, T_, float(kd_lambda), mode, int(threshold is not None),
              float(threshold or 0.0), stats.data_ptr(), out.data_ptr(), w.data_ptr(), sisdr.data_ptr(), gest.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    return out, w, sisdr, gest, stats


def test_two_source_instantiation_equals_the_two_source_kernels(golden):
    """fqss_kd_loss_n at S = 2 against fqss_kd_loss / fqss_kd_loss_per_sample / fqss_pit_sisdr_loss on tests/golden/loss.npz: loss, w,
    SI-SDR at the kernels' tolerances, dL/d est at rtol 1e-6 (the same fp64 coefficients feed the same fp32 map), and the moment
    rows slot for slot"""
    from fqss_amd import kernels as K
    g = golden("loss")
    est, fest, tgt = (T(g[k]).cuda() for k in ("est", "fest", "tgt"))
    cases = [(0, est, fest, tgt, lambda: K.kd_loss(est, fest, tgt, 0.1), None),
             (2, est, tgt, tgt, lambda: (lambda o, s, ge: (o, None, s, ge))(*K.pit_sisdr_loss(est, tgt)), None)]
    for Bm, th in ((1, None), (2, None), (2, -30.0), (2, 1e9)):
        e, f, t = est[:Bm].contiguous(), fest[:Bm].contiguous(), tgt[:Bm].contiguous()
        cases.append((1, e, f, t, lambda e=e, f=f, t=t, th=th: K.kd_loss(e, f, t, 0.1, per_sample=True, threshold=th), th))
    for mode, e, f, t, old, th in cases:
        out0, w0, sisdr0, gest0 = old()
        out, w, sisdr, gest, _ = _loss_n(e, f, t, mode, threshold=th)
        msg = f"mode {mode} B={len(e)} th={th}"
        np.testing.assert_allclose(out.cpu().numpy(), out0.cpu().numpy(), rtol=1e-5, err_msg=msg)
        if w0 is not None:
            np.testing.assert_allclose(w.cpu().numpy(), w0.cpu().numpy(), rtol=2e-5, err_msg=msg)
        np.testing.assert_allclose(sisdr.cpu().numpy(), sisdr0.cpu().numpy(), atol=1e-3, err_msg=msg)
        np.testing.assert_allclose(gest.cpu().numpy(), gest0.cpu().numpy(), rtol=1e-6, err_msg=msg)
    # the golden itself, through the new kernels
    out, w, sisdr, gest, _ = _loss_n(est, fest, tgt, 0)
    np.testing.assert_allclose(out[0].item(), g["loss"], rtol=1e-5)
    np.testing.assert_allclose(w.cpu().numpy(), g["w"], rtol=2e-5)
    np.testing.assert_allclose(sisdr.cpu().numpy(), -g["sdrqs"], atol=1e-3)
    # moments: same slots, same launch shape; only the order of the atomics differs
    from fqss_amd import _lib
    m0 = K.kd_moments(est, fest, tgt).cpu()
    m = torch.empty(3, K.KD_STATS_STRIDE_N, device="cuda", dtype=torch.float64)
    _lib.call("fqss_kd_moments_n", est.data_ptr(), fest.data_ptr(), tgt.data_ptr(), 3, 2, est.shape[-1], m.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    np.testing.assert_allclose(m.cpu().numpy()[:, :24], m0.numpy()[:, :24], rtol=1e-12, atol=1e-12)      # fp64 sums of ~400 terms below 0.1, re-ordered


def test_refused_arguments_leave_the_outputs_untouched():
    """every FQSS_REQUIRE of fqss_kd_loss_n / fqss_kd_moments_n: FQSS_EINVAL, and nothing is written"""
    from fqss_amd import _lib, kernels as K
    einval = _lib.CONSTANTS["FQSS_EINVAL"]
    B, S, T_ = 3, 3, 300
    x = torch.zeros(B, S, T_, device="cuda")
    nan = lambda *shape, dt=torch.float32: torch.full(shape, float("nan"), device="cuda", dtype=dt)
    stats, out, w, sisdr, gest = nan(1025, K.KD_STATS_STRIDE_N, dt=torch.float64), nan(4), nan(1025), nan(1025), nan(B, S, T_)
    st = torch.cuda.current_stream().cuda_stream
    ok = dict(est=x.data_ptr(), fest=x.data_ptr(), tgt=x.data_ptr(), B=B, S=S, T=T_, lam=0.1, mode=0, ut=0, th=0.0, stats=stats.data_ptr(),
              out=out.data_ptr(), w=w.data_ptr(), sisdr=sisdr.data_ptr(), gest=gest.data_ptr())
    order = ("est", "fest", "tgt", "B", "S", "T", "lam", "mode", "ut", "th", "stats", "out", "w", "sisdr", "gest")
    bad = [{k: None} for k in ("est", "fest", "tgt", "stats", "out", "w", "sisdr")]
    bad += [dict(S=0), dict(S=4), dict(B=0), dict(B=1025), dict(T=0), dict(mode=-1), dict(mode=3), dict(mode=1, B=2)]
    for change in bad:
        a = dict(ok, **change)
        assert _lib.query("fqss_kd_loss_n", *[a[k] for k in order], st) == einval, change
    assert "B must be 1 or n_src" in _lib.load().fqss_last_error().decode()
    morder = ("est", "fest", "tgt", "B", "S", "T", "stats")
    for change in [{k: None} for k in ("est", "fest", "tgt", "stats")] + [dict(S=0), dict(S=4), dict(B=0), dict(B=1025), dict(T=0)]:
        a = dict(ok, **change)
        assert _lib.query("fqss_kd_moments_n", *[a[k] for k in morder], st) == einval, change
    torch.cuda.synchronize()
    for t in (stats, out, w, sisdr, gest):
        assert bool(torch.isnan(t).all())
    # the accepted call right after still works (mode 1 at B = n_src)
    s, e, f = N.batch3(3, T_)
    assert _lib.query("fqss_kd_loss_n", e.cuda().data_ptr(), f.cuda().data_ptr(), s.cuda().data_ptr(), 3, 3, T_, 0.1, 1, 0, 0.0, stats.data_ptr(),
                      out.data_ptr(), w.data_ptr(), sisdr.data_ptr(), gest.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gest).all())
    with pytest.raises(NotImplementedError, match="1 to 3"):
        K.kd_loss(torch.zeros(1, 4, 64, device="cuda"), torch.zeros(1, 4, 64, device="cuda"), torch.zeros(1, 4, 64, device="cuda"), 0.1)


def _rel(a, b):
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-12))


def test_tiny_three_source_training_eager_and_replayed():
    """steps 1-2 against the oracle; 51 eager steps and one quantizing step; then, from that state with lr = 0, one eager step +
    capture + two replays against a second stepper's three eager steps on the same inputs (the comparison of
    tests/test_gpu_kdstep_path.py: output 1e-4, loss / KD 1e-5, weights 2.3e-4, gradient norm 1e-4, every gradient 2e-3); one eager
    step of the teacher-free mode"""
    from fqss_amd import data, ops
    from fqss_amd.runtime import KDTrainStep
    from tests.test_gpu_model import _leave_observer
    model, step = N.check_tiny_training("cuda")                      # steps 1, 2
    x, tgt = (t.cuda() for t in data.synth_batch(2, 800, seed=0, n_src=3))
    for s in range(3, 53):                                           # the observer phase ends at step 50
        r = step(x, tgt)
    torch.cuda.synchronize()
    assert np.isfinite(r["loss"].item()) and r["est"].shape == (2, 3, 800) and bool(torch.isfinite(r["est"]).all())
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    batches = [tuple(t.cuda() for t in data.synth_batch(2, 800, seed=100 + i, n_src=3)) for i in range(3)]

    def run(replay):
        m, f = N.tiny_pair("cuda")
        m.load_state_dict(state, strict=True)
        _leave_observer(m)
        st = KDTrainStep(m, f, kd_lambda=0.1, lr=0.0, clip=5.0)
        res = []
        with ops.poison_carriers(True):
            for i, (xb, tb) in enumerate(batches):
                if replay and i == 1:
                    st.capture(xb, tb, warmup=0)
                    assert st._graphs is not None
                if replay and i >= 1:
                    st.arena.flat_g.fill_(float("nan"))              # the replay must rewrite every gradient
                r = st(xb, tb)
                torch.cuda.synchronize()
                res.append((dict(est=r["est"].cpu().numpy(), loss=r["loss"].item(), kd=r["kd"].item(), w=r["w"].cpu().numpy(),
                                 gnorm=r["gnorm"].item()), {n: p.grad.detach().cpu().numpy().copy() for n, p in m.named_parameters()}))
        return res

    eager, replayed = run(False), run(True)
    for i in (1, 2):
        (a, ga), (b, gb) = replayed[i], eager[i]
        np.testing.assert_allclose(a["est"], b["est"], rtol=1e-4, atol=2e-6)
        for k in ("loss", "kd"):
            np.testing.assert_allclose(a[k], b[k], rtol=1e-5)
        np.testing.assert_allclose(a["w"], b["w"], rtol=2.3e-4)
        np.testing.assert_allclose(a["gnorm"], b["gnorm"], rtol=1e-4)
        assert all(np.isfinite(v).all() for v in ga.values())
        for n, v in ga.items():
            assert _rel(v, gb[n]) <= 2e-3 or np.linalg.norm(gb[n]) < 1e-7, (i, n, _rel(v, gb[n]))
    # kd_lambda = 0: the teacher-free PIT SI-SDR loss
    m0, f0 = N.tiny_pair("cuda")
    r0 = KDTrainStep(m0, f0, kd_lambda=0.0, lr=1e-3, clip=5.0)(x, tgt)
    want = O.neg_sisdr_pit(r0["est"].cpu().double(), tgt.cpu().double())
    np.testing.assert_allclose(r0["loss"].item(), want.item(), rtol=1e-5)
    assert np.isfinite(r0["gnorm"].item()) and r0["gnorm"].item() > 0.0


@pytest.mark.parametrize("B,Ci,Co,M,add", [(2, 128, 1536, 130, False), (1, 48, 1040, 77, True), (1, 128, 2064, 64, True)])
def test_qgemm_dgrad_above_1024_output_channels(B, Ci, Co, M, add):
    """the mask conv of three sources x 512 filters has 1536 output channels: fqss_qpw_bwd_x(_add) runs its reduction in parts of at
    most 1024 rows (1536 = 768 + 768; 1040 = 528 + 512: a ragged last part; 2064 = 3 x 688) and adds the fork's other gradient once.
    Against W_q^T gz in float64 at the tolerance of tests/test_gpu_kernels.py::test_qgemm_fwd_bwd."""
    from fqss_amd import kernels as K
    gen = torch.Generator().manual_seed(Ci + Co)
    w = torch.randn(Co, Ci, 1, generator=gen) * Ci ** -0.5
    wlo = -(torch.rand(Co, 1, 1, generator=gen) * 0.2 + 0.05)
    whi = torch.rand(Co, 1, 1, generator=gen) * 0.2 + 0.05
    wq = O.weight_quantize(w, wlo, whi)

    def padded(t):
        d = K.empty_act(tuple(t.shape), "cuda")
        d.copy_(t)
        return d
    wc = K.wq_codes(w.cuda().contiguous(), wlo.cuda(), whi.cuda())
    gz = torch.randn(B, Co, M, generator=gen)
    other = torch.randn(B, Ci, M, generator=gen) if add else None
    gx = K.qpw_bwd_x(padded(gz), wc, add=padded(other) if add else None)
    ref = torch.einsum("oc,bom->bcm", wq[:, :, 0].double(), gz.double()) + (other.double() if add else 0.0)
    np.testing.assert_allclose(gx.cpu().double().numpy(), ref.numpy(), rtol=1e-5, atol=2e-6 * float(ref.abs().max()))


def test_train_cli_three_sources(tmp_path):
    """`python -m fqss_amd.train -env asteroid -y configs/convtasnet_3spks_8k_synthetic.yaml`, one epoch of 55 steps of 1 s at batch 2:
    the observer phase ends inside it, so the epoch finishes as hipGraph replays"""
    import yaml
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "convtasnet_3spks_8k_synthetic.yaml")))
    assert conf["model_cfg"]["n_src"] == 3 and conf["dataset_cfg"]["n_src"] == 3
    conf["work_dir"] = str(tmp_path / "run")
    conf["dataset_cfg"].update(segment=1, steps_per_epoch=55, val_steps=2)
    conf["training_cfg"].update(epochs=1, batch_size=2)
    yml = tmp_path / "cfg.yaml"
    yml.write_text(yaml.safe_dump(conf))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "fqss_amd.train", "-env", "asteroid", "-y", str(yml)], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    recs = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(recs) == 1 and recs[0]["launch"] == "hipGraph replay", recs
    assert np.isfinite(recs[0]["loss"]) and np.isfinite(recs[0]["val_loss"])
    assert os.path.exists(os.path.join(conf["work_dir"], "best_model.pth"))
