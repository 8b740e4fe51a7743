"""Resuming an interrupted run, without a GPU: the asteroid env on the CPU backend (`--use_cpu`, configs/convtasnet_2spks_8k_cpu.yaml)
stopped after one epoch and resumed must end exactly where the uninterrupted run ends -- the CPU backend is bit-reproducible, so
equality is the bar -- and the checkpoint file's own promises: atomic replacement, `weights_only=True`, refusal of an arena of another
layout, refusal of another world size while the ranks still hold their own observer ranges."""
import os
import subprocess

import pytest
import torch
import yaml

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


def _cfg(tmp_path, name, epochs, resume=None):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "convtasnet_2spks_8k_cpu.yaml")))
    cfg["work_dir"] = str(tmp_path / name)
    cfg["dataset_cfg"].update(steps_per_epoch=1, val_steps=1)
    cfg["training_cfg"].update(epochs=epochs)
    if resume is not None:
        cfg["training_cfg"]["resume"] = resume
    yml = tmp_path / f"{name}_{epochs}.yaml"
    yml.write_text(yaml.safe_dump(cfg))
    return str(yml), cfg["work_dir"]


def test_cpu_run_resumed_after_one_epoch_equals_the_uninterrupted_run(tmp_path, cpu_backend):
    from fqss_amd import checkpoint
    from fqss_amd.train_env.asteroid_librimix import asteroid_librimix_trainer as T
    yml_a, dir_a = _cfg(tmp_path, "a", 2)
    hist_a = T.train(yml_a, "cpu")
    yml_b1, dir_b = _cfg(tmp_path, "b", 1, resume="auto")       # auto with nothing to resume: a fresh start
    hist_b1 = T.train(yml_b1, "cpu")
    assert len(hist_b1) == 1 and os.path.exists(os.path.join(dir_b, "checkpoint.pth"))
    # the relaunch: no key in the YAML, the `resume=` argument that `--resume` hands over; its `pretrained` file has gone missing since --
    # student and teacher come from the checkpoint
    yml_b2, _ = _cfg(tmp_path, "b", 2)
    cfg = yaml.safe_load(open(yml_b2))
    assert "resume" not in cfg["training_cfg"]
    cfg["training_cfg"]["pretrained"] = str(tmp_path / "moved_away.pth")
    open(yml_b2, "w").write(yaml.safe_dump(cfg))
    hist_b = T.train(yml_b2, "cpu", resume="auto")
    assert [h["epoch"] for h in hist_a] == [h["epoch"] for h in hist_b] == [0, 1]
    for ha, hb in zip(hist_a, hist_b):
        for k in ("loss", "val_loss", "lr"):
            assert ha[k] == hb[k], (k, ha, hb)
    sd_a = torch.load(os.path.join(dir_a, "latest_model.pth"), weights_only=True)
    sd_b = torch.load(os.path.join(dir_b, "latest_model.pth"), weights_only=True)
    assert len(sd_a) == 948 and list(sd_a) == list(sd_b)
    differ = [k for k in sd_a if not torch.equal(sd_a[k], sd_b[k])]
    assert not differ, (len(differ), differ[:5])
    ck_a = checkpoint.load_training_state(os.path.join(dir_a, "checkpoint.pth"))
    ck_b = checkpoint.load_training_state(os.path.join(dir_b, "checkpoint.pth"))
    assert ck_a["format"] == "fqss-train-v1" and ck_a["trainer"]["epoch"] == ck_b["trainer"]["epoch"] == 2
    for k in ("flat_p", "exp_avg", "exp_avg_sq", "t0", "step_t"):
        assert torch.equal(ck_a["step"]["arena"][k], ck_b["step"]["arena"][k]), k
    assert ck_a["step"]["arena"]["host_step"] == ck_b["step"]["arena"]["host_step"] == 2
    assert ck_a["step"]["act_quantizers"] == ck_b["step"]["act_quantizers"] and ck_a["step"]["weight_quantizers"] == ck_b["step"]["weight_quantizers"]
    # 2 training + 2 validation forwards; the weight observers ran on the first
    assert {q["n_iter"] for q in ck_a["step"]["act_quantizers"].values()} == {4}
    assert not any(q["observer_mode"] for q in ck_a["step"]["weight_quantizers"].values())
    assert all(torch.equal(v, ck_b["teacher"][k]) for k, v in ck_a["teacher"].items())
    # a run whose stored epoch already equals `epochs` returns its stored history and touches nothing
    stamp = {f: os.stat(os.path.join(dir_b, f)).st_mtime_ns for f in os.listdir(dir_b)}
    again = T.train(yml_b2, "cpu", resume=os.path.join(dir_b, "checkpoint.pth"))
    assert again == ck_b["trainer"]["history"] and len(again) == 2
    assert stamp == {f: os.stat(os.path.join(dir_b, f)).st_mtime_ns for f in os.listdir(dir_b)}


def test_train_cli_has_the_resume_flag(monkeypatch):
    import sys
    from fqss_amd import train as cli
    for argv, want in ((["--resume"], "auto"), (["--resume", "/x/checkpoint.pth"], "/x/checkpoint.pth"), ([], None)):
        monkeypatch.setattr(sys, "argv", ["train.py", "-env", "asteroid", "-y", "cfg.yaml"] + argv)
        assert cli.argument_handler().resume == want


def test_resume_path_auto_and_explicit(tmp_path):
    from fqss_amd import checkpoint
    assert checkpoint.resume_path(None, str(tmp_path)) is None
    assert checkpoint.resume_path("auto", str(tmp_path)) is None
    (tmp_path / "checkpoint.pth").write_bytes(b"x")
    assert checkpoint.resume_path("auto", str(tmp_path)) == str(tmp_path / "checkpoint.pth")
    assert checkpoint.resume_path(str(tmp_path / "checkpoint.pth"), "/nowhere") == str(tmp_path / "checkpoint.pth")
    with pytest.raises(FileNotFoundError):
        checkpoint.resume_path(str(tmp_path / "missing.pth"), str(tmp_path))


# ---- the file, without any network ---------------------------------------------------------------------------------------------
class _Net(torch.nn.Module):
    """a convolution weight, one activation quantizer, one weight quantizer, one persistent buffer"""

    def __init__(self, width=4):
        from fqss_amd.quantization.qat import qat_quant as QQ
        super().__init__()
        self.conv = torch.nn.Conv1d(2, width, 3)
        self.aq = QQ.GradientActivationFakeQuantize(True)
        self.wq = QQ.GradientWeightFakeQuantize(True, (width, 2, 3))
        self.register_buffer("running", torch.arange(3.0))


def _step(comm=None, width=4, seed=0):
    from fqss_amd.runtime import KDTrainStep
    torch.manual_seed(seed)
    return KDTrainStep(_Net(width), _Net(width), kd_lambda=0.1, lr=1e-3, comm=comm)


def _scribble(step, seed):
    """arbitrary but recognisable training state, as a run would have left it"""
    g = torch.Generator().manual_seed(seed)
    a = step.arena
    for t in (a.flat_p, a.exp_avg, a.exp_avg_sq):
        t.copy_(torch.randn(t.shape, generator=g))
    a.step_t.fill_(7)
    a._host_step = 7
    o = a.offsets[a.names.index("conv.weight")]
    a.t0[o:o + step.model.conv.weight.numel()] = 3
    a._inactive = [(p, off) for p, off in a._inactive if p is not step.model.conv.weight]
    step.model.aq.n_iter, step.model.wq.observer_mode, step.model.aq.sign = 28, False, False
    step.model.running.add_(5.0)
    step.lr = 2.5e-4


def test_checkpoint_file_round_trip_weights_only_and_atomic(tmp_path, cpu_backend, monkeypatch):
    from fqss_amd import checkpoint
    path = str(tmp_path / "run" / "checkpoint.pth")
    src = _step()
    _scribble(src, 1)
    torch.manual_seed(123)
    import random
    import numpy as np
    random.seed(5)
    np.random.seed(6)
    checkpoint.save_training_state(path, src, dict(epoch=3, best=float("inf"), history=[{"epoch": 0, "loss": 1.5, "launch": "eager"}]), src.fmodel)
    want = (random.random(), float(np.random.uniform()), torch.rand(3))
    # tensors and plain values only
    raw = torch.load(path, map_location="cpu", weights_only=True)
    assert raw["format"] == "fqss-train-v1" and set(raw) == {"format", "step", "trainer", "teacher", "rng"}
    ck = checkpoint.load_training_state(path)
    dst = _step(seed=9)                       # another initialisation: everything must come from the file
    assert not torch.equal(dst.arena.flat_p, src.arena.flat_p)
    p_ptr, g_ptr = dst.model.conv.weight.data_ptr(), dst.model.conv.weight.grad.data_ptr()
    ts = checkpoint.restore(ck, dst, dst.fmodel)
    assert ts == dict(epoch=3, best=float("inf"), history=[{"epoch": 0, "loss": 1.5, "launch": "eager"}])
    assert (random.random(), float(np.random.uniform())) == want[:2] and torch.equal(torch.rand(3), want[2])
    for k in ("flat_p", "exp_avg", "exp_avg_sq", "step_t", "t0"):
        assert torch.equal(getattr(dst.arena, k), getattr(src.arena, k)), k
    # loaded INTO the flat buffers: the parameter views are the same memory and show the stored values
    assert dst.model.conv.weight.data_ptr() == p_ptr and dst.model.conv.weight.grad.data_ptr() == g_ptr
    assert torch.equal(dst.model.conv.weight, src.model.conv.weight) and torch.equal(dst.model.running, src.model.running)
    assert dst.arena._host_step == 7 and dst.lr == 2.5e-4
    assert (dst.model.aq.n_iter, dst.model.aq.observer_mode, dst.model.aq.sign, dst.model.wq.observer_mode) == (28, True, False, False)
    # _inactive rebuilt from t0: everything but the convolution weight still waits for its first gradient
    name_at = dict(zip(dst.arena.offsets, dst.arena.names))
    assert sorted(name_at[o] for _, o in dst.arena._inactive) == sorted(n for n in dst.arena.names if n != "conv.weight")
    assert all(torch.equal(v, dst.fmodel.state_dict()[k]) for k, v in src.fmodel.state_dict().items())
    assert (dst.tables, dst._graphs, dst._tgraph, dst._ahead, dst._eager_q) == (None, None, None, None, 0)
    # a failure between the temporary write and the replace: the old file stays, loadable, and no temporary file is left behind
    before = open(path, "rb").read()

    def boom(a, b):
        raise OSError("killed between write and replace")
    monkeypatch.setattr(checkpoint.os, "replace", boom)
    _scribble(src, 2)
    with pytest.raises(OSError, match="killed between"):
        checkpoint.save_training_state(path, src, dict(epoch=4), src.fmodel)
    monkeypatch.undo()
    assert open(path, "rb").read() == before and os.listdir(os.path.dirname(path)) == ["checkpoint.pth"]
    assert checkpoint.load_training_state(path)["trainer"]["epoch"] == 3
    # a student-only file is named for what it is
    torch.save(src.model.state_dict(), str(tmp_path / "latest_model.pth"))
    with pytest.raises(ValueError, match="not a training-state checkpoint"):
        checkpoint.load_training_state(str(tmp_path / "latest_model.pth"))


def test_arena_of_another_layout_is_refused(cpu_backend):
    src, other = _step(), _step(width=8)
    with pytest.raises(ValueError, match="layout does not match"):
        other.load_state_dict(src.state_dict())
    with pytest.raises(ValueError, match="layout does not match"):
        other.arena.load_state_dict(src.arena.state_dict())
    # same sizes under other names: refused too
    twin = _step()
    sd = src.arena.state_dict()
    sd["layout"]["names"][0] = "elsewhere.weight"
    with pytest.raises(ValueError, match="first differing name"):
        twin.arena.load_state_dict(sd)


def _two_rank_comm(rank, peer_rows):
    """a Comm of world 2 whose all_gather answers with this rank's tensor and a given peer's (no process group)"""
    from fqss_amd.parallel import Comm
    comm = Comm(rank=rank, world=2)
    comm.all_gather = lambda t: [t.clone(), peer_rows(t)] if rank == 0 else [peer_rows(t), t.clone()]
    comm.barrier = lambda: None
    return comm


def test_state_written_before_the_range_sync_keeps_every_ranks_ranges(cpu_backend):
    def peer(t):         # the other rank: ranges (-2, 3), n_iter 31
        out = t.clone()
        out[:, 0:1] = torch.tensor([-2.0]).view(torch.int32)
        out[:, 1:2] = torch.tensor([3.0]).view(torch.int32)
        out[:, 2] = 31
        return out
    src = _step(comm=_two_rank_comm(0, peer))
    assert not src._ranges_synced
    src.model.aq.min_range.data.fill_(-0.25)
    src.model.aq.max_range.data.fill_(0.75)
    src.model.aq.n_iter = 30
    sd = src.state_dict()
    assert sd["world"] == 2 and tuple(sd["rank_ranges"].shape) == (2, 1, 3) and sd["ranges_synced"] is False
    for rank, (lo, hi, n) in enumerate([(-0.25, 0.75, 30), (-2.0, 3.0, 31)]):
        dst = _step(comm=_two_rank_comm(rank, peer), seed=4)
        dst.load_state_dict(sd)
        assert (dst.model.aq.min_range.item(), dst.model.aq.max_range.item(), dst.model.aq.n_iter) == (lo, hi, n)
        assert not dst._ranges_synced
        # the range parameters are arena views: the rank's own values sit in its flat parameter buffer
        o = dst.arena.offsets[dst.arena.names.index("aq.min_range")]
        assert dst.arena.flat_p[o].item() == lo
    with pytest.raises(ValueError, match="world size 2"):
        _step().load_state_dict(sd)
    # after the sync one copy serves any world size
    src._ranges_synced = True
    sd = src.state_dict()
    assert sd["rank_ranges"] is None
    one = _step(seed=4)
    one.load_state_dict(sd)
    assert one.model.aq.min_range.item() == -0.25 and one._ranges_synced


# ---- one copy, any world size: the arena's ORDER follows the gradient buckets -----------------------------------------------------
def _convtasnet_step(comm=None, seed=0, **kw):
    """a four-block ConvTasNet: at world > 1 (or with `buckets`) its arena is laid out in backward-segment order (fqss_segments)"""
    from fqss_amd.runtime import KDTrainStep
    from fqss_amd.smoke import build_pair
    model, fmodel = build_pair("cpu", seed, n_spks=2, kernel_size=16, stride=8, n_filters=32, bn_chan=16, hid_chan=32, n_blocks=4, n_repeats=1)
    return KDTrainStep(model, fmodel, kd_lambda=0.1, lr=1e-3, comm=comm, **kw)


def _scribble_arena(step, seed, n_iter):
    """recognisable state per parameter: random values and moments, a first-gradient step of its own for every second parameter"""
    g = torch.Generator().manual_seed(seed)
    a = step.arena
    for i, (p, o) in enumerate(zip(a.params, a.offsets)):
        for t in (a.flat_p, a.exp_avg, a.exp_avg_sq):
            t[o:o + p.numel()] = torch.randn(p.numel(), generator=g)
        if i % 2:
            a.t0[o:o + p.numel()] = i
    a._inactive = [(p, o) for i, (p, o) in enumerate(zip(a.params, a.offsets)) if not i % 2]
    a.step_t.fill_(60)
    a._host_step = 60
    for _, m in step._quantizers()[0]:
        m.n_iter = n_iter
    for _, m in step._quantizers()[1]:
        m.observer_mode = False


def _by_name(step):
    a = step.arena
    return {n: tuple(t[o:o + p.numel()].clone() for t in (a.flat_p, a.exp_avg, a.exp_avg_sq, a.t0))
            for n, p, o in zip(a.names, a.params, a.offsets)}


@pytest.mark.parametrize("way", ["2 ranks -> 1 rank", "1 rank -> 2 ranks", "4 buckets -> 2 buckets"])
def test_state_written_after_the_range_sync_serves_another_world_size(cpu_backend, way):
    """a relaunch on fewer (or more) GPUs: the file's arena is in another order than this launch's, and is loaded by parameter name"""
    two = lambda: _two_rank_comm(0, lambda t: t.clone())
    src_comm, dst_comm, src_kw, dst_kw = {"2 ranks -> 1 rank": (two(), None, {}, {}), "1 rank -> 2 ranks": (None, two(), {}, {}),
                                          "4 buckets -> 2 buckets": (two(), two(), dict(buckets=4), dict(buckets=2))}[way]
    src = _convtasnet_step(src_comm, seed=0, **src_kw)
    _scribble_arena(src, 3, n_iter=50)
    src._ranges_synced = True                                     # past the observer phase: the ranks have averaged
    sd = src.state_dict()
    assert sd["rank_ranges"] is None
    dst = _convtasnet_step(dst_comm, seed=7, **dst_kw)
    assert dst.arena.layout() != sd["arena"]["layout"], "the two launches must order their arenas differently for this test to mean anything"
    assert sorted(dst.arena.names) == sorted(sd["arena"]["layout"]["names"])
    ptrs = [p.data_ptr() for p in dst.arena.params]
    dst.load_state_dict(sd)
    assert [p.data_ptr() for p in dst.arena.params] == ptrs
    want, got = _by_name(src), _by_name(dst)
    for n in want:
        assert all(torch.equal(u, v) for u, v in zip(want[n], got[n])), n
    # the parameters themselves (arena views) and, through them, the student's state_dict
    sd_src, sd_dst = src.model.state_dict(), dst.model.state_dict()
    assert list(sd_src) == list(sd_dst) and all(torch.equal(v, sd_dst[k]) for k, v in sd_src.items())
    name_at = dict(zip(dst.arena.offsets, dst.arena.names))
    assert sorted(name_at[o] for _, o in dst.arena._inactive) == sorted(n for i, n in enumerate(src.arena.names) if not i % 2)
    assert dst.arena._host_step == 60 and int(dst.arena.step_t) == 60 and dst._ranges_synced
    # padding between parameters: no moments, no clock
    used = torch.zeros(dst.arena.numel, dtype=torch.bool)
    for p, o in zip(dst.arena.params, dst.arena.offsets):
        used[o:o + p.numel()] = True
    assert not dst.arena.exp_avg[~used].any() and (dst.arena.t0[~used] == 2 ** 31 - 1).all()
    # and back: what this launch writes, the first reads
    back = _convtasnet_step(src_comm, seed=9, **src_kw)
    back.load_state_dict(dst.state_dict())
    assert all(torch.equal(u, v) for n in want for u, v in zip(want[n], _by_name(back)[n]))


def test_one_rank_file_resumed_on_two_ranks_synchronises_only_inside_the_observer_phase(cpu_backend):
    two = lambda: _two_rank_comm(0, lambda t: t.clone())
    for n_iter, due in ((28, True), (50, False)):
        src = _convtasnet_step()
        _scribble_arena(src, 5, n_iter=n_iter)
        sd = src.state_dict()
        assert sd["world"] == 1 and sd["ranges_synced"] is True and sd["rank_ranges"] is None
        dst = _convtasnet_step(two(), seed=2)
        dst.load_state_dict(sd)
        # inside the phase the ranks observe their own shards from here on: the one-time averaging is still due.  Past it every rank
        # starts from the same ranges: nothing to average
        assert dst._ranges_synced == (not due) and dst.can_capture() == (not due)
