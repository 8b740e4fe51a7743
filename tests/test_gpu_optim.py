"""The optimizer family on the device: fqss_optim_clip / fqss_ema_update (csrc/train_ops.hip) against torch.optim and fp64 on the CPU --
the bodies, shapes and bounds of tests/optim_common.py, which tests/test_optim_cpu.py runs on the CPU backend and whose docstring says
where the Adam-L2 case and the data come from --, a ConvTasNet step under AdamW with an EMA copy eagerly and replayed from the
hipGraphs, and the htdemucs env with AdamW and a batch-level and an epoch-level EMA copy."""
import math
import os
import sys

import pytest
import torch

from tests import optim_common as C
from tests.test_accum_cpu import ab, make_step, settle
from tests.test_gpu_model import TINY

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# shift 1: every buffer one float past a 16-B boundary -- the kernel's scalar-access form; 0: its 16-B form with a scalar last group
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", C.SIZES)
@pytest.mark.parametrize("case", list(C.CASES))
def test_optim_clip_vs_torch_optim(case, n, shift):
    C.check_vs_torch(case, n, shift)


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", C.SIZES)
def test_adam_without_decay_gives_the_bits_of_adam_clip(n, shift):
    C.check_adam_bits(n, shift)


@pytest.mark.parametrize("case", list(C.CASES))
def test_per_parameter_clocks_and_untouched_elements(case):
    C.check_clocks(case)


@pytest.mark.parametrize("case", ["adamw_1e-2", "sgd_momentum", "sgd_nesterov"])
def test_slot_table_equals_three_param_groups(case):
    C.check_slot_table(case)


@pytest.mark.parametrize("on_device", [False, True], ids=["host_w", "device_count"])
@pytest.mark.parametrize("n,shift", [(100003, 0), (100003, 1), (1, 0), (65, 0)])
def test_ema_update_vs_fp64(n, shift, on_device):
    C.check_ema(n, on_device, shift)


@pytest.mark.parametrize("name", list(C.REFUSED))
def test_optim_clip_refusals(name):
    C.check_refusal(name)


def test_ema_update_refusals():
    C.check_ema_refusals()


# ---- the step --------------------------------------------------------------------------------------------------------------------------
KW = dict(optimizer="adamw", weight_decay=0.01, ema_decays=(0.999,))


def _pair(**kw):
    """two identically built steps in ONE state past the observer phase (tests/test_accum_cpu.py pair_of_steps, under `kw`)"""
    one = settle(make_step("cuda", TINY, **kw), "cuda")
    two = make_step("cuda", TINY, **kw)
    sd = one.state_dict()
    two.load_state_dict(sd)
    one.load_state_dict(sd)
    return one, two


def _state(step):
    a = step.arena
    return {"flat_p": a.flat_p, "exp_avg": a.exp_avg, "exp_avg_sq": a.exp_avg_sq, "step_t": a.step_t, "ema": step.ema[0],
            "ema_count": step.ema_count}


def test_adamw_with_an_ema_copy_replays_bit_equal_to_eager(monkeypatch):
    """4 eager steps against 2 eager steps + 2 replays of the graphs captured in between: a learning rate, a bias correction or an EMA
    weight frozen into the graph would part the two (w = 1 / count changes with every update)"""
    monkeypatch.setenv("FQSS_DETERMINISTIC", "1")       # bit-reproducible gradients: what is compared is the update
    A, B = ab("cuda")
    eager, graph = _pair(**KW)
    assert eager.det is not None and eager._optim_block()["kind"] == "adamw" and len(eager.ema) == 1
    start = eager.ema[0].clone()
    for x, tgt in (A, B, A, B):
        eager(x, tgt)
    assert eager._graphs is None
    for x, tgt in (A, B):
        graph(x, tgt)
    graph.capture(A[0], A[1], warmup=0)
    assert graph._graphs is not None
    for x, tgt in (A, B):
        graph(x, tgt)
    torch.cuda.synchronize()
    want, got = _state(eager), _state(graph)
    differ = [k for k in want if not torch.equal(want[k], got[k])]
    assert not differ, differ
    # six updates since the copy was made (two settling calls ran before the state was shared; the shared state carries their count)
    count = 0.0
    for _ in range(6):
        count = count * 0.999 + 1.0
    assert eager.ema_count.item() == count and int(eager.arena.step_t) == 6
    assert not torch.equal(eager.ema[0], start) and not torch.equal(eager.ema[0], eager.arena.flat_p)
    # the copy in and out of the model: same addresses, same bits after
    p0 = graph.arena.params[0]
    before, copy, addr = graph.arena.flat_p.clone(), graph.ema[0].clone(), p0.data_ptr()
    with graph.ema_swap(0):
        assert torch.equal(graph.arena.flat_p, copy) and torch.equal(graph.ema[0], before) and p0.data_ptr() == addr
        assert torch.equal(graph.ema_state(0)[graph.arena.names[0]].reshape(-1), before[:p0.numel()])
    assert torch.equal(graph.arena.flat_p, before) and torch.equal(graph.ema[0], copy) and p0.data_ptr() == addr


def test_ema_advances_once_per_accumulation_window():
    A, B = ab("cuda")
    step, _ = _pair(accumulate=2, **KW)
    c0, t0 = step.ema_count.item(), int(step.arena.step_t)
    step(*A)
    assert step.pending == 1 and step.ema_count.item() == c0 and int(step.arena.step_t) == t0
    step(*B)
    assert step.pending == 0 and step.ema_count.item() == c0 * 0.999 + 1.0 and int(step.arena.step_t) == t0 + 1


def test_htdemucs_env_with_adamw_and_ema_copies(tmp_path, monkeypatch):
    import yaml
    from fqss_amd import checkpoint
    from fqss_amd.train_env.htdemucs_musdbhq import train as T
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "htdemucs_synthetic.yaml")))
    conf["work_dir"] = str(tmp_path / "run")
    conf["dset"].update(segment=0.05, sources=["a", "b"], steps_per_epoch=2, valid_steps=1)
    conf.update(epochs=1, batch_size=2, weights=[1.0, 1.0])
    conf["htdemucs"] = dict(nfft=2048, channels=8, bottom_channels=16, t_layers=3, t_heads=2, t_weight_decay=0.05)
    conf["ema"] = dict(batch=[0.9], epoch=[0.5])
    conf["optim"].update(optim="adamw", weight_decay=0.01)
    yml = tmp_path / "cfg.yaml"
    yml.write_text(yaml.safe_dump(conf))
    monkeypatch.setattr(sys, "argv", ["train.py", "+device=cuda", f"+yml_path={yml}"])
    hist = T.main()
    valid = hist[0]["valid"]
    losses = {k: valid[k]["loss"] for k in ("main", "ema_batch_0", "ema_epoch_0")}
    assert len(hist) == 1 and all(math.isfinite(v) for v in losses.values()), losses
    assert valid["bname"] == min(losses, key=losses.get) and valid["loss"] == min(losses.values()) == valid["best"]
    ck = checkpoint.load_training_state(os.path.join(conf["work_dir"], "checkpoint.pth"))["step"]
    assert ck["optim"]["kind"] == "adamw" and ck["optim"]["weight_decay"] == 0.01
    # the cross-transformer's parameters carry their own decay, whatever optim.weight_decay says
    own = ck["optim"]["param_decay"]
    assert own and all(n.startswith("crosstransformer.") for n in own) and set(own.values()) == {0.05}
    assert ck["ema"]["kinds"] == ["batch", "epoch"] and ck["ema"]["decays"] == [0.9, 0.5]
    assert ck["ema"]["count"].tolist() == [0.9 * 1.0 + 1.0, 1.0]       # two updates of the batch copy, one of the epoch copy
    assert int(ck["arena"]["step_t"]) == 2
