"""The optimizer family without a GPU: fqss_optim_clip / fqss_ema_update on the CPU backend against torch.optim on the CPU
(foreach=False), and the asteroid env under `--use_cpu` with AdamW and SGD-momentum, stopped, resumed and compared bit for bit.
The bodies are tests/optim_common.py's, which tests/test_gpu_optim.py runs on the HIP kernels.

Adam with L2 decay and the bound (rtol 1e-6, atol 1e-7, the bound of test_adam_clip_vs_torch).  Where g + wd * p cancels, the update
m / (sqrt(v) + eps) amplifies whatever rounded on the way to that sum -- the clip coefficient alone differs by an ulp between torch
(fp32 norm) and the kernel (fp64 sum of squares) -- so one unlucky element can put ANY fp32 implementation outside the bound, torch's
included.  Which element cancels is an accident of the data, so the data was chosen by the reference's own error, measured so:
n = 100003, p = randn(seed 1), g = 0.05 * randn(seed 2), clip 5.0, 5 steps of torch.optim.Adam(lr=1e-3, weight_decay=wd,
foreach=False), once on the fp32 tensors and once on their fp64 copies; figure = max |a - b| / (atol + rtol |b|) over the elements
after the fifth step, fp32 result against fp64 result (1.0 = at the bound).
    steps 2 and 4 scaled by 3.0:     wd 1e-3: 3.06    wd 1e-2: 0.48      (torch's own fp32 result is outside the bound at 1e-3)
    steps 1, 3 and 5 scaled by 3.0:  wd 1e-3: 0.24    wd 1e-2: 0.40
So "every second step" is the first, third and fifth here, and the Adam-L2 case runs at wd = 1e-3; the kernel then sits at 0.41 of
the bound or less against torch's fp32 result on every step.  AdamW (wd 1e-2 and 0.1) and SGD (lr 1e-2, wd 1e-2, momentum 0.9, with
and without nesterov) have no such cancellation in a denominator and run as stated.  The slot-table case, whose decays reach 0.1, runs
on AdamW and SGD (SGD forms g + wd * p on the branch Adam uses) and not on Adam-L2: 64 elements per decay say nothing about a
cancellation that one element in 10^5 meets."""
import os
import subprocess

import pytest
import torch
import yaml

from tests import optim_common as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def cpu_backend():
    from fqss_amd import _lib
    if not os.path.exists(_lib.CPU_SO_PATH):
        subprocess.check_call(["make", "-C", os.path.dirname(_lib.CPU_SO_PATH)])
    prev = _lib.BACKEND
    _lib.set_backend("cpu")
    yield
    _lib.set_backend(prev)


@pytest.mark.parametrize("n", C.SIZES)
@pytest.mark.parametrize("case", list(C.CASES))
def test_optim_clip_vs_torch_optim(case, n, cpu_backend):
    C.check_vs_torch(case, n)


@pytest.mark.parametrize("n", C.SIZES)
def test_adam_without_decay_gives_the_bits_of_adam_clip(n, cpu_backend):
    C.check_adam_bits(n)


@pytest.mark.parametrize("case", list(C.CASES))
def test_per_parameter_clocks_and_untouched_elements(case, cpu_backend):
    C.check_clocks(case)


@pytest.mark.parametrize("case", ["adamw_1e-2", "sgd_momentum", "sgd_nesterov"])
def test_slot_table_equals_three_param_groups(case, cpu_backend):
    C.check_slot_table(case)


@pytest.mark.parametrize("on_device", [False, True], ids=["host_w", "device_count"])
@pytest.mark.parametrize("n", [100003, 1, 65])
def test_ema_update_vs_fp64(n, on_device, cpu_backend):
    C.check_ema(n, on_device)


@pytest.mark.parametrize("name", list(C.REFUSED))
def test_optim_clip_refusals(name, cpu_backend):
    C.check_refusal(name)


def test_ema_update_refusals(cpu_backend):
    C.check_ema_refusals()


# ---- end to end: the asteroid env on the CPU backend ---------------------------------------------------------------------------------
def _cfg(tmp_path, name, epochs, optim):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "convtasnet_2spks_8k_cpu.yaml")))
    cfg["work_dir"] = str(tmp_path / name)
    cfg["dataset_cfg"].update(steps_per_epoch=1, val_steps=1)
    cfg["training_cfg"].update(epochs=epochs)
    cfg["training_cfg"]["optim"].update(optim)
    yml = tmp_path / f"{name}_{epochs}.yaml"
    yml.write_text(yaml.safe_dump(cfg))
    return str(yml), cfg["work_dir"]


ADAMW = dict(optimizer="adamw", weight_decay=0.01)
SGD = dict(optimizer="sgd", momentum=0.9)


def _resumed_equals_uninterrupted(tmp_path, optim, tag):
    from fqss_amd import checkpoint
    from fqss_amd.train_env.asteroid_librimix import asteroid_librimix_trainer as T
    yml_a, dir_a = _cfg(tmp_path, tag + "_a", 2, optim)
    hist_a = T.train(yml_a, "cpu")
    yml_b1, dir_b = _cfg(tmp_path, tag + "_b", 1, optim)
    T.train(yml_b1, "cpu")
    yml_b2, _ = _cfg(tmp_path, tag + "_b", 2, optim)
    hist_b = T.train(yml_b2, "cpu", resume="auto")
    assert [h["epoch"] for h in hist_a] == [h["epoch"] for h in hist_b] == [0, 1]
    for ha, hb in zip(hist_a, hist_b):
        for k in ("loss", "val_loss", "lr"):
            assert ha[k] == hb[k], (k, ha, hb)
    ck_a = checkpoint.load_training_state(os.path.join(dir_a, "checkpoint.pth"))
    ck_b = checkpoint.load_training_state(os.path.join(dir_b, "checkpoint.pth"))
    for k in ("flat_p", "exp_avg", "exp_avg_sq", "t0", "step_t"):
        assert torch.equal(ck_a["step"]["arena"][k], ck_b["step"]["arena"][k]), k
    assert ck_a["step"]["optim"] == ck_b["step"]["optim"] and "ema" not in ck_a["step"]
    return ck_a


@pytest.fixture(scope="module")
def adamw_runs(tmp_path_factory):
    """the AdamW runs, once for the tests below: (the uninterrupted run's checkpoint, the path of that file)"""
    from fqss_amd import _lib
    prev = _lib.BACKEND
    _lib.set_backend("cpu")
    try:
        tmp = tmp_path_factory.mktemp("adamw")
        return _resumed_equals_uninterrupted(tmp, ADAMW, "adamw"), os.path.join(str(tmp / "adamw_a"), "checkpoint.pth")
    finally:
        _lib.set_backend(prev)


def test_adamw_run_resumes_bit_equal_and_its_file_names_the_optimizer(adamw_runs):
    ck, _ = adamw_runs
    assert ck["step"]["optim"] == {"kind": "adamw", "weight_decay": 0.01, "momentum": 0.0, "nesterov": False, "param_decay": {}}
    assert ck["step"]["arena"]["exp_avg_sq"].abs().max() > 0


def test_sgd_momentum_run_resumes_bit_equal_and_refuses_the_adamw_file(tmp_path, cpu_backend, adamw_runs):
    from fqss_amd.train_env.asteroid_librimix import asteroid_librimix_trainer as T
    ck = _resumed_equals_uninterrupted(tmp_path, SGD, "sgd")
    assert ck["step"]["optim"]["kind"] == "sgd" and ck["step"]["optim"]["momentum"] == 0.9
    assert ck["step"]["arena"]["exp_avg"].abs().max() > 0 and ck["step"]["arena"]["exp_avg_sq"].abs().max() == 0    # the buffer; never v
    # the AdamW run's file into an SGD step: refused, both named
    yml_s, _ = _cfg(tmp_path, "s", 3, SGD)
    with pytest.raises(ValueError, match=r"'adamw'.*'sgd'"):
        T.train(yml_s, "cpu", resume=adamw_runs[1])


def test_default_checkpoint_has_no_optim_or_ema_key_and_other_names_are_refused(tmp_path, cpu_backend):
    from fqss_amd import checkpoint
    from fqss_amd.train_env.asteroid_librimix import asteroid_librimix_trainer as T
    yml, work = _cfg(tmp_path, "d", 1, {})
    T.train(yml, "cpu")
    step = checkpoint.load_training_state(os.path.join(work, "checkpoint.pth"))["step"]
    assert "optim" not in step and "ema" not in step
    yml, _ = _cfg(tmp_path, "r", 1, dict(optimizer="rmsprop"))
    with pytest.raises(NotImplementedError, match="adam, adamw, sgd"):
        T.train(yml, "cpu")


def test_ema_copies_travel_through_the_step_state(cpu_backend):
    """a step with a batch-level and an epoch-level copy: state_dict -> a fresh step -> the same copies and counts; another EMA list
    is refused"""
    from fqss_amd.runtime import KDTrainStep
    from tests.test_resume_cpu import _Net

    def make(**kw):
        torch.manual_seed(0)
        return KDTrainStep(_Net(), _Net(), kd_lambda=0.1, lr=1e-3, optimizer="adamw", weight_decay=0.01, **kw)

    src = make(ema_decays=(0.9,), ema_epoch_decays=(0.5,))
    src.arena.flat_g.copy_(C.rnd(src.arena.numel, 7, 0.05))
    src.arena.t0.zero_()
    for _ in range(3):
        src._optimize(activate=False)
    src.ema_epoch_update()
    assert src.ema_count.tolist() == [0.9 * (0.9 * 1 + 1) + 1, 1.0]
    assert torch.equal(src.ema[1], src.arena.flat_p) and not torch.equal(src.ema[0], src.arena.flat_p)
    assert torch.equal(src.ema_state(0)["conv.weight"].reshape(-1), src.ema[0][:src.model.conv.weight.numel()])
    before, copy, addr = src.arena.flat_p.clone(), src.ema[0].clone(), src.model.conv.weight.data_ptr()
    with src.ema_swap(0):
        assert torch.equal(src.arena.flat_p, copy) and torch.equal(src.ema[0], before)
        assert torch.equal(src.model.conv.weight.reshape(-1), copy[:24]) and src.model.conv.weight.data_ptr() == addr
    assert torch.equal(src.arena.flat_p, before) and torch.equal(src.ema[0], copy) and src.model.conv.weight.data_ptr() == addr
    sd = src.state_dict()
    assert sd["ema"]["kinds"] == ["batch", "epoch"] and sd["ema"]["decays"] == [0.9, 0.5]
    dst = make(ema_decays=(0.9,), ema_epoch_decays=(0.5,))
    dst.load_state_dict(sd)
    assert all(torch.equal(a, b) for a, b in zip(src.ema, dst.ema)) and torch.equal(src.ema_count, dst.ema_count)
    with pytest.raises(ValueError, match="EMA"):
        make(ema_decays=(0.99,)).load_state_dict(sd)


def test_param_decay_fills_the_slot_table_and_the_default_step_stays_on_adam_clip(cpu_backend, monkeypatch):
    from fqss_amd import kernels as K
    from fqss_amd.runtime import KDTrainStep
    from tests.test_resume_cpu import _Net

    def make(**kw):
        torch.manual_seed(0)
        return KDTrainStep(_Net(), _Net(), kd_lambda=0.1, lr=1e-3, **kw)

    step = make(optimizer="adamw", weight_decay=0.01, param_decay={"conv.bias": 0.1})
    a = step.arena
    want = torch.full((a.numel // 64,), 0.01)
    o = a.offsets[a.names.index("conv.bias")]
    want[o // 64:(o + step.model.conv.bias.numel() + 63) // 64] = 0.1
    assert torch.equal(step._wd_slot, want) and step._optim_block()["param_decay"] == {"conv.bias": 0.1}
    assert make(optimizer="adamw", weight_decay=0.01, param_decay={"conv.bias": 0.01})._wd_slot is None      # nobody departs: no table
    assert make(param_decay={"conv.bias": 0.1})._optim_block()["kind"] == "adam"         # adam with a decayed group is not the default run
    with pytest.raises(ValueError, match="nowhere"):
        make(param_decay={"nowhere": 0.1})
    for bad in (dict(optimizer="rmsprop"), dict(weight_decay=-1.0), dict(optimizer="sgd", momentum=1.0),
                dict(optimizer="sgd", nesterov=True), dict(optimizer="adam", momentum=0.9), dict(ema_decays=(1.0,))):
        with pytest.raises(ValueError):
            make(**bad)
    # the decayed slot decays, the others do not: one AdamW update on a zero gradient moves only conv.bias (p *= 1 - lr * wd)
    step = make(optimizer="adamw", weight_decay=0.0, param_decay={"conv.bias": 0.1})
    step.arena.t0.zero_()
    before = step.arena.flat_p.clone()
    step._optimize(activate=False)
    moved = (step.arena.flat_p != before).nonzero().flatten().tolist()
    assert moved and set(moved) <= set(range(o, o + step.model.conv.bias.numel()))
    assert torch.equal(step.arena.flat_p[moved], before[moved] * torch.tensor(1.0 - 1e-3 * 0.1, dtype=torch.float32))
    # the default configuration never reaches fqss_optim_clip
    default = make()
    assert default._optim_block() is None and default._wd_slot is None and not default.ema

    def refuse(*a, **k):
        raise AssertionError("the default step must stay on fqss_adam_clip")

    monkeypatch.setattr(K, "optim_clip", refuse)
    monkeypatch.setattr(K, "ema_update", refuse)
    default._optimize(activate=False)
    assert int(default.arena.step_t) == 1
