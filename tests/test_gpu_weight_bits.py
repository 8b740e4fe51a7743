"""Weight quantizers at 2 to 8 bits (`weight_n_bits`) on the HIP path: the width-taking kernels (csrc/fq.hip k_wq_fwd / k_wq_bwd,
csrc/qgemm.hip k_wq_codes, csrc/multi.hip k_wq_multi_fwd / k_wq_multi_bwd reading the width per descriptor) against the reference's own
numbers (tests/golden/fq_w_bits.npz, tiny_step_w4.npz; tools/make_goldens_wbits.py) and the oracle, then W4A8 through everything that sits
on top of them: training step, QuantTables, hipGraph replay, serving, export, the trainer CLI."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle.fqss_oracle as O
from tests import helpers_wbits as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = H.T


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    yield


def close(got, want, rtol=2e-5, atol=None, msg=""):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    atol = atol if atol is not None else rtol * float(want.abs().max())
    err = float((got - want).abs().max())
    assert err <= atol + rtol * float(want.abs().max()), (msg, err, float(want.abs().max()))


# ------------------------------------------------------------------------------------------------ kernels
def test_fq_w_bits_goldens_bit_exact():
    """the reference's GradientWeightFakeQuantize at n = 2 .. 7 on k_wq_fwd / k_wq_bwd: idx, y, gw bit for bit, gmin / gmax at the gate
    of test_golden_fq_w; at n = 8 the same entry points give fq_w.npz bit for bit"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "fq_w_bits.npz"))
    H.check_fq_w_bits(g, "cuda")
    g8 = np.load(os.path.join(ROOT, "tests", "golden", "fq_w.npz"))
    for i in range(int(g8["n_cases"])):
        H.check_fq_w_case(g8, "", 8, i, "cuda")


@pytest.mark.parametrize("n", [2, 4, 6])
@pytest.mark.parametrize("shape,axis", [((512, 128, 1), 0), ((512, 1, 3), 0), ((512, 1, 16), 1)])
def test_fq_w_full_size_vs_oracle(n, shape, axis):
    from fqss_amd import kernels as K
    gen = torch.Generator().manual_seed(shape[0] + axis + 100 * n)
    w = torch.randn(*shape, generator=gen) * 0.1
    rs = [1] * 3
    rs[axis] = shape[axis]
    lo = -(torch.rand(*rs, generator=gen) * 0.3 + 0.01)
    hi = torch.rand(*rs, generator=gen) * 0.3 + 0.01
    y, idx = K.wq_fwd(w.cuda(), axis, lo.cuda(), hi.cuda(), want_idx=True, n_bits=n)
    idx_ref = O.weight_indices(w, lo, hi, n_bits=n)
    assert int(idx_ref.min()) == -2 ** (n - 1) and int(idx_ref.max()) == 2 ** (n - 1) - 1      # (the case does clip on both sides)
    assert torch.equal(idx.cpu(), idx_ref)
    assert torch.equal(y.cpu(), O.weight_quantize(w, lo, hi, n_bits=n))


@pytest.mark.parametrize("Co,Ci", [(128, 64), (64, 256)])
def test_wq_codes_at_4_bits(Co, Ci):
    """k_wq_codes at n = 4: dw * idx is k_wq_fwd's y bit for bit, rw the row sums, idxT the transpose; the int8 row GEMM on those codes
    agrees with the fp32-equivalent GEMM on dw * idx at 2e-5 (the pattern of test_qrow_kernel_exact_integer_sums)"""
    from fqss_amd import kernels as K
    gen = torch.Generator().manual_seed(Co + Ci)
    w = (torch.randn(Co, Ci, generator=gen) * 0.2).cuda()
    lo = (-(w.abs().amax(1, keepdim=True)) * 0.9).contiguous()
    hi = (w.abs().amax(1, keepdim=True) * 0.95).contiguous()
    wc = K.wq_codes(w, lo, hi, n_bits=4)
    y, idx = K.wq_fwd(w, 0, lo, hi, want_idx=True, n_bits=4)
    assert int(wc.idx.min()) == -8 and int(wc.idx.max()) == 7
    assert torch.equal(wc.idx, idx) and torch.equal(wc.idxT, idx.t().contiguous())
    assert torch.equal(wc.dw[:, None] * wc.idx.float(), y)
    assert torch.equal(wc.rw.cpu(), wc.idx.cpu().float().sum(1))
    assert not torch.equal(wc.idx, K.wq_codes(w, lo, hi).idx)          # (and the default is still the 8-bit grid)
    R = 777
    xc = torch.randint(0, 256, (R, Ci), generator=torch.Generator().manual_seed(52), dtype=torch.uint8).cuda()
    xlo, xhi = torch.tensor([-1.3], device="cuda"), torch.tensor([2.1], device="cuda")
    b = torch.randn(Co, generator=gen).cuda()
    z = K.qrow_fwd(xc, wc, b, xlo, xhi)
    x = ((xhi - xlo) / 255.0) * xc.float() + xlo
    close(z, K.rowlin_fwd(x, (wc.dw[:, None] * wc.idx.float()).contiguous(), b), 2e-5)


# ------------------------------------------------------------------------------------------------ QuantTables
def _w4(golden):
    return golden("tiny_step_w4")


def _tables_vs_modules(build, x, tgt):
    """the body of test_batched_quant_tables_match_per_module_path: same state, same batch -> same loss, same flat gradient"""
    from fqss_amd.runtime import KDTrainStep
    grads, losses = [], []
    for batched in (False, True):
        model, fmodel = build()
        step = KDTrainStep(model, fmodel)
        if not batched:
            step._quant_tables = lambda: None
        r = step._fwd_bwd(x, tgt)
        assert (step.tables is not None) == batched
        if batched:
            widths = sorted({int(r_[17]) for r_ in step.tables.wq_table.cpu().tolist()})
            assert widths == sorted({m.n_bits for m, _, _, _ in step.tables.weights}), widths
        losses.append(r["loss"].item())
        grads.append(step.arena.flat_g.clone())
    np.testing.assert_allclose(losses[0], losses[1], rtol=1e-6)
    err = float((grads[0] - grads[1]).abs().max())
    assert err <= 2e-5 * float(grads[0].abs().max()) + 1e-7, err
    return widths


def test_batched_quant_tables_match_per_module_path_w4a8(golden):
    g = _w4(golden)

    def build():
        model, fmodel = H.tiny_pair_w4(g, "cuda", prefix="s50.post_sd.")
        H.leave_observer(model)
        return model, fmodel
    assert _tables_vs_modules(build, T(g["x"]).cuda(), T(g["tgt"]).cuda()) == [4]


def test_batched_quant_tables_with_mixed_widths(golden):
    """one model, three widths, set by hand before the tables are built: TCN at 4 bits with every skip_conv -- the second member of a
    res|skip pair, whose codes share one concatenated image -- at 6, encoder / bottleneck / mask conv / decoder at 8"""
    from fqss_amd.quantization.qat import qat_quant as QQ
    g = _w4(golden)

    def build():
        model, fmodel = H.tiny_pair_w4(g, "cuda", prefix="s50.post_sd.")
        H.leave_observer(model)
        H.mixed_widths(model, tcn_bits=4, other_bits=8)
        n6 = 0
        for name, m in model.named_modules():
            if isinstance(m, QQ.GradientWeightFakeQuantize) and ".skip_conv." in name:
                m.n_bits, n6 = 6, n6 + 1
        assert n6 > 0
        return model, fmodel
    assert _tables_vs_modules(build, T(g["x"]).cuda(), T(g["tgt"]).cuda()) == [4, 6, 8]


def test_dptnet_batched_quantizer_tables_w4a8():
    """the DPTNet table test at W4A8: conv, LinearQ, attention-projection and LSTM weight quantizers from the tables == per layer"""
    from fqss_amd.quantization.qat import qat_quant as QQ
    from fqss_amd.quantization.qat.models.dptnetq import DPTNetQ
    from fqss_amd.quantization.qat.models.load_model import quantize_model
    from tests.helpers_segments import check_batched_tables
    tiny = dict(n_spks=2, kernel_size=2, enc_dim=16, feature_dim=8, hidden_dim=12, layer=2, segment_size=10)

    def build():
        torch.manual_seed(0)
        model = DPTNetQ(**tiny)
        fmodel = copy.deepcopy(model)
        model = quantize_model(model, H.qcfg(4))
        assert all(m.n_bits == 4 for m in model.modules() if isinstance(m, QQ.GradientWeightFakeQuantize))
        return model.cuda().train(), fmodel.cuda().eval()
    x, tgt = O.synth_batch(1, 4000, seed=3)
    check_batched_tables(build, x.cuda(), tgt.cuda(), 36, step_kw=dict(kd_lambda=0.1, clip=0.0))


# ------------------------------------------------------------------------------------------------ the tiny W4A8 model vs the reference
def test_tiny_w4a8_training_vs_reference_goldens(golden, capsys):
    with capsys.disabled():
        H.check_tiny_training_w4(_w4(golden), "cuda")


def _idx_stats(y, y_ref, lo, hi):
    delta = (hi - lo) / 255.0
    a = np.rint((y - lo) / delta)
    b = np.rint((y_ref - lo) / delta)
    return float(np.mean(a != b)), float(np.abs(a - b).max())


def test_tiny_w4a8_step51_teacher_forced(golden, capsys):
    """state after 50 steps, each LayerQ fed the reference's recorded input of step 51 (the first quantizing step): worst bin distance
    <= 1, mismatching share <= 1e-3 -- the caps of test_tiny_step51_teacher_forced"""
    g = _w4(golden)
    model, _ = H.tiny_pair_w4(g, "cuda", prefix="s50.post_sd.")
    H.leave_observer(model)
    tot, bad, worst = 0, 0, 0.0
    with torch.no_grad():
        for name in g["layer_names"]:
            name = str(name)
            if name.endswith("residual_error_block"):
                continue   # called with the decoder's tensors; covered through `decoder`
            mod = dict(model.named_modules())[name]
            ins, j = [], 0
            while f"s51.actin{j}.{name}" in g.files:
                ins.append(T(g[f"s51.actin{j}.{name}"]).cuda())
                j += 1
            out = mod(*ins).cpu().numpy()
            ref = g[f"s51.act.{name}"]
            sd = mod.state_dict()
            keys = ["activation_fake_quantize"] + (["activation_fake_quantize_residual"] if name == "decoder" else [])
            for ch, key in enumerate(keys):
                o, r = (out[ch], ref[ch]) if name == "decoder" else (out, ref)
                frac, dmax = _idx_stats(o, r, float(sd[key + ".min_range"]), float(sd[key + ".max_range"]))
                tot += o.size
                bad += frac * o.size
                worst = max(worst, dmax)
    with capsys.disabled():
        print(f"step 51 teacher-forced at W4A8: worst bin distance {worst}, mismatching share {bad / tot:.3e} of {tot}")
    assert worst <= 1, worst
    assert bad / tot <= 1e-3, (bad, tot)


def test_tiny_w4a8_step51_end_to_end_from_reference_state(golden, capsys):
    """free-running forward of step 51 from the reference's step-50 state.  The loss tolerance at 4 bits comes from the fixture:
    max(0.05 dB, 3 |s51.loss - s51.loss_f64|) -- the floor is the 8-bit gate, the factor 3 allows for the GPU's summation order on top
    of the reference's own fp32 / fp64 sensitivity at this state"""
    from fqss_amd import kernels as K
    g = _w4(golden)
    model, fmodel = H.tiny_pair_w4(g, "cuda", prefix="s50.post_sd.")
    H.leave_observer(model)
    x, tgt = T(g["x"]).cuda(), T(g["tgt"]).cuda()
    with torch.no_grad():
        est = model(x)
        fest = fmodel(x)
    out, w, sisdr, _ = K.kd_loss(est, fest, tgt, 0.1, want_grad=False)
    tol = max(0.05, 3.0 * abs(float(g["s51.loss"]) - float(g["s51.loss_f64"])))
    with capsys.disabled():
        print(f"step 51 free-running at W4A8: loss {out[0].item():.5f}, reference {float(g['s51.loss']):.5f} (float64 "
              f"{float(g['s51.loss_f64']):.5f}), tolerance used {tol:.4f} dB")
    np.testing.assert_allclose(fest.cpu().numpy(), g["s51.fest"], rtol=1e-4, atol=2e-6)
    assert abs(out[0].item() - float(g["s51.loss"])) <= tol, (out[0].item(), float(g["s51.loss"]), tol)


def test_hipgraph_replay_matches_eager_w4a8(golden):
    """the body of test_hipgraph_replay_matches_eager on the W4A8 pair"""
    from fqss_amd.runtime import KDTrainStep
    g = _w4(golden)
    x, tgt = T(g["x"]).cuda(), T(g["tgt"]).cuda()
    runs = []
    for use_graph in (False, True):
        model, fmodel = H.tiny_pair_w4(g, "cuda", prefix="s50.post_sd.")
        H.leave_observer(model)
        step = KDTrainStep(model, fmodel)
        losses = [step(x, tgt)["loss"].item()]          # eager step (all Adam clocks start)
        if use_graph:
            step.capture(x, tgt, warmup=1)
        else:
            step(x, tgt)
        for _ in range(3):
            losses.append(step(x, tgt)["loss"].item())
        runs.append((losses, step.arena.flat_p.clone()))
    (l0, p0), (l1, p1) = runs
    np.testing.assert_allclose(l0[0], l1[0], rtol=1e-6)
    np.testing.assert_allclose(l0[1:], l1[1:], atol=0.05)          # dB; chaotic after the first quantized update
    assert float((p0 - p1).abs().max()) < 5e-3


# ------------------------------------------------------------------------------------------------ serving, export, CLI
def test_infer_runner_bit_identical_w4a8(golden):
    from fqss_amd.quantization.qat.models.load_model import enable_observer
    from fqss_amd.runtime import InferRunner
    g = _w4(golden)
    m, _ = H.tiny_pair_w4(g, "cuda", prefix="s50.post_sd.")
    enable_observer(m, False)
    m.eval()
    run = InferRunner(m)
    mix = T(g["x"]).cuda()
    xs = [mix[:1, :, :640].contiguous(), mix[:, :, :800].contiguous()]
    with torch.no_grad():
        want = [m(x).clone() for x in xs]
    for _ in range(2):
        for x, w in zip(xs, want):
            assert torch.equal(run(x), w)
    assert len(run._graphs) == 2
    # and the 4-bit grid is what it ran on: the same state at 8 bits separates differently
    m8, _ = H.build_pair("cuda", H.qcfg(8), **H.TINY)
    m8.load_state_dict(m.state_dict())
    enable_observer(m8, False)
    with torch.no_grad():
        assert not torch.equal(m8.eval()(xs[1]), want[1])


def test_export_integer_state_at_4_bits(golden):
    from fqss_amd.quantization.qat import qat_quant as QQ
    from fqss_amd.quantization.qat.qat_utils import weight_quantizer_owners
    g = _w4(golden)
    m, _ = H.tiny_pair_w4(g, "cuda", prefix="s50.post_sd.")
    H.leave_observer(m)
    st = QQ.export_integer_state(m)
    names = {id(mod): n for n, mod in m.named_modules()}
    owners = weight_quantizer_owners(m)
    assert len(owners) >= 10
    for wqm, w, pname in owners:
        e = st[names[id(wqm)]]
        assert (e["quant_min"], e["quant_max"]) == (-8, 7), pname
        t = QQ.TorchWeightFakeQuantize(wqm)
        lo, hi = wqm.min_range.detach().cpu(), wqm.max_range.detach().cpu()
        y_ref, codes_ref, scales_ref = O.weight_export(w.detach().cpu(), lo, hi, wqm.axis, n_bits=4)
        assert torch.equal(t.scales.cpu(), scales_ref) and torch.equal(e["scales"], scales_ref), pname
        codes = t.integer(w.detach())
        assert codes.dtype == torch.int8 and torch.equal(codes.cpu().int(), codes_ref), pname
        assert torch.equal(t(w.detach()).cpu(), y_ref), pname
    assert all(e["quant_max"] == 255 for e in st.values() if "scale" in e)


def test_train_cli_w4_synthetic_config(tmp_path):
    """`python -m fqss_amd.train -env asteroid -y configs/convtasnet_2spks_8k_synthetic_w4.yaml`, shortened like
    test_asteroid_env_trains_and_exports shortens the 8-bit config: exits 0 and prints finite losses"""
    import yaml
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "convtasnet_2spks_8k_synthetic_w4.yaml")))
    assert conf["model_cfg"]["quantization"]["weight_n_bits"] == 4 and conf["model_cfg"]["quantization"]["act_n_bits"] == 8
    ref = yaml.safe_load(open(os.path.join(ROOT, "configs", "convtasnet_2spks_8k_synthetic.yaml")))
    assert conf["work_dir"] != ref["work_dir"]
    conf["work_dir"] = str(tmp_path / "run")
    conf["dataset_cfg"].update(segment=0.5, steps_per_epoch=4, val_steps=2)
    conf["training_cfg"].update(epochs=2, batch_size=2)
    yml = tmp_path / "cfg.yaml"
    yml.write_text(yaml.safe_dump(conf))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "fqss_amd.train", "-env", "asteroid", "-y", str(yml)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    hist = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{") and '"loss"' in l]
    assert len(hist) == 2 and all(np.isfinite(h["loss"]) and np.isfinite(h["val_loss"]) for h in hist), p.stdout[-2000:]
    sd = torch.load(os.path.join(conf["work_dir"], "best_model.pth"), weights_only=True)
    assert len(sd) == 948 and all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
