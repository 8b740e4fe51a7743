"""GPU: the objectives of the htdemucs solver beside L1 + distillation -- a teacher-free step under `loss_kind="mse"` against autograd
through F.mse_loss, eagerly and as a hipGraph replay, and the trainer under configs/htdemucs_synthetic_mse.yaml.  Margins: those of
tests/test_gpu_htdemucs.py (loss 1e-6 relative on the same model output, gradients 1e-2 by norm)."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_htdemucs import QCFG, TINY_KW, T, _sd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_against_autograd(step, res, g_step, mix, src):
    # loss against F.mse_loss at the step's own output; the arena against the backward of the same dataflow from autograd's d mse / d est
    leaf = res["est"].clone().requires_grad_(True)
    (want := F.mse_loss(leaf, src)).backward()
    np.testing.assert_allclose(res["loss"].item(), want.item(), rtol=1e-6)
    assert math.isfinite(res["nsdr"].item())
    _, est, _, cuts = step._forward_loss(mix, src)
    for k in range(step._nseg(cuts)):
        step._backward_segment(k, est, leaf.grad, cuts)
    g_ref = step.arena.flat_g
    assert float(g_ref.norm()) > 0 and float((g_step - g_ref).norm()) <= 1e-2 * float(g_ref.norm())


def test_mse_step_without_teacher_matches_autograd_eager_and_replayed(golden):
    from fqss_amd.quantization.qat.models.htdemucsq import HTDemucsQ
    from fqss_amd.quantization.qat.models.load_model import quantize_model
    from fqss_amd.runtime import KDTrainStep
    g = golden("hd_tiny_step")
    mix, src = T(g["mix"]).cuda(), T(g["src"]).cuda()
    model = quantize_model(HTDemucsQ(**TINY_KW), QCFG)
    model.load_state_dict(_sd(g, "sd0."), strict=True)
    model = model.cuda().train()
    step = KDTrainStep(model, None, kd_lambda=0.0, lr=3e-4, clip=0.0, loss="l1_sdr", loss_kind="mse")
    assert step.teacher is None
    step._fwd_bwd(mix, src)                                     # call 1 observes the weights: calls 2 and 3 run the same network
    res = step._fwd_bwd(mix, src)                               # observer phase, eager
    check_against_autograd(step, res, step.arena.flat_g.clone(), mix, src)
    with torch.no_grad():
        for _ in range(47):
            model(mix)
    step(mix, src)                                              # the eager quantizing step a capture needs
    step.capture(mix, src, warmup=0)
    res = step.replay_fwd_bwd(mix, src)
    check_against_autograd(step, res, step.arena.flat_g.clone(), mix, src)
    assert math.isfinite(step(mix, src)["loss"].item()) and step._graphs is not None
    assert step._tgraph is None and step._tstream is None, "a teacher-free step opens no teacher stream and records no teacher graph"


def test_trainer_epoch_under_mse_without_teacher_selects_by_nsdr_and_resumes(tmp_path, monkeypatch):
    import yaml
    from fqss_amd import checkpoint
    from fqss_amd.train_env.htdemucs_musdbhq import train as Tr
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "htdemucs_synthetic_mse.yaml")))
    assert conf["optim"]["loss"] == "mse" and conf["kd_lambda"] == 0 and conf["test"]["metric"] == "nsdr"
    conf["work_dir"] = str(tmp_path / "run")
    conf["dset"].update(segment=0.05, sources=["a", "b"], steps_per_epoch=2, valid_steps=1)
    conf.update(epochs=1, batch_size=2, weights=[1.0, 2.0])
    conf["htdemucs"] = dict(nfft=2048, channels=8, bottom_channels=16, t_layers=3, t_heads=2)
    conf["ema"] = dict(batch=[0.9], epoch=[])
    yml = tmp_path / "cfg.yaml"
    yml.write_text(yaml.safe_dump(conf))
    monkeypatch.setattr(sys, "argv", ["train.py", "+device=cuda", f"+yml_path={yml}"])
    hist = Tr.main()
    train, valid = hist[0]["train"], hist[0]["valid"]
    # mse: reco is the weighted mean of the items' root mean squares, loss of their mean squares (Jensen: reco^2 <= loss)
    assert train["reco"] != train["loss"] and 0 < train["reco"] ** 2 <= train["loss"] * (1 + 1e-6)
    for rec in (valid, valid["main"], valid["ema_batch_0"]):
        assert all(math.isfinite(rec[k]) for k in ("loss", "reco", "nsdr", "nsdr_a", "nsdr_b")), rec
        np.testing.assert_allclose(rec["nsdr"], (rec["nsdr_a"] + 2.0 * rec["nsdr_b"]) / 3.0, rtol=1e-6)
    scores = {k: valid[k]["nsdr"] for k in ("main", "ema_batch_0")}
    assert valid["bname"] == max(scores, key=scores.get) and valid["nsdr"] == max(scores.values()) == valid["best"]
    assert os.path.exists(os.path.join(conf["work_dir"], "best.th"))
    ck = checkpoint.load_training_state(os.path.join(conf["work_dir"], "checkpoint.pth"))
    assert ck["step"]["objective"] == {"loss_kind": "mse", "teacher": False} and ck["teacher"] is None and ck["trainer"]["metric"] == "nsdr"
    monkeypatch.setattr(sys, "argv", ["train.py", "+device=cuda", f"+yml_path={yml}", "epochs=2", "resume=auto"])
    hist2 = Tr.main()       # a second epoch from the checkpoint: the new history keys and the teacher-free step round-trip
    assert len(hist2) == 2 and hist2[0] == hist[0] and math.isfinite(hist2[1]["valid"]["nsdr"]) and hist2[1]["valid"]["best"] >= valid["best"]
