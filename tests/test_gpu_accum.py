"""Gradient accumulation on the device: fqss_grad_accum bit for bit against torch, a window of two micro-batches against the same two
gradients summed by hand -- bit-equal under FQSS_DETERMINISTIC=1, eagerly and replayed from the hipGraphs; within the summation-order
bound with the default fp32 atomics --, the exchange schedule on a forced one-rank communicator, and the update counts of the
speechbrain and htdemucs environments."""
import math
import os
import subprocess
import sys

import pytest
import torch

from tests.test_accum_cpu import ab, check_grad_accum, pair_of_steps, reference_window, same, snapshot
from tests.test_gpu_model import TINY

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNMOVED = ("flat_p", "exp_avg", "exp_avg_sq", "step_t", "t0", "host_step")


def test_grad_accum_equals_torch_bit_for_bit_on_the_device():
    check_grad_accum("cuda")


def test_window_of_two_is_bit_equal_in_deterministic_mode_eager_and_replayed(monkeypatch):
    monkeypatch.setenv("FQSS_DETERMINISTIC", "1")
    A, B = ab("cuda")
    ref, got = pair_of_steps("cuda", TINY, accumulate=2)
    assert ref.det is not None and got.det is not None and got.arena.acc is not None
    # eagerly
    before = snapshot(got)
    want = reference_window(ref, (True, True), (A, B))
    got(*A)
    assert not same(before, snapshot(got), UNMOVED) and got.pending == 1
    with pytest.raises(RuntimeError):
        got.capture(A[0], A[1], warmup=0)                 # not inside a window
    got(*B)
    assert got.pending == 0 and not same(want, snapshot(got)), same(want, snapshot(got))
    assert int(want["step_t"]) == int(before["step_t"]) + 1 and not torch.equal(want["flat_p"], before["flat_p"])
    # captured at the window boundary, the next window replayed: per-segment graphs and the clip + Adam graph, no one-graph step
    got.capture(A[0], A[1], warmup=0)
    assert got._graphs is not None and getattr(got, "_graph_all", None) is None
    before = snapshot(got)
    want = reference_window(ref, (True, True), (A, B))
    got.arena.acc.fill_(float("nan"))
    got.arena.flat_g.fill_(float("nan"))
    got(*A)
    assert not same(before, snapshot(got), UNMOVED) and got.pending == 1
    got(*B)
    assert got.pending == 0 and not same(want, snapshot(got)), same(want, snapshot(got))
    assert torch.isfinite(got.arena.flat_p).all() and int(want["step_t"]) == int(before["step_t"]) + 1


def test_window_of_two_with_fp32_atomics_stays_within_the_summation_order_bound(monkeypatch):
    """default mode: a gradient is one fp32 summation order of many.  4e-6 of its norm is the whole-arena bound
    tests/test_gpu_kdstep_path.py holds between two orders of one gradient; the window's sum holds two gradients, each one order away
    from its reference: 8e-6 * (|gA| + |gB|)"""
    monkeypatch.delenv("FQSS_DETERMINISTIC", raising=False)
    A, B = ab("cuda")
    ref, got = pair_of_steps("cuda", TINY, accumulate=2)
    assert got.det is None
    ref._step_eager(*A)
    gA = ref.arena.flat_g.double().clone()
    ref._step_eager(*B)
    gB = ref.arena.flat_g.double().clone()
    ra = got(*A)
    rb = got(*B)
    a = got.arena
    assert got.pending == 0 and int(a.step_t) == int(ref.arena.step_t) + 1
    for t in (a.flat_g, a.flat_p, a.exp_avg, a.exp_avg_sq, a.gnorm, ra["loss"], rb["loss"]):
        assert torch.isfinite(t).all()
    err, scale = float((a.flat_g.double() - (gA + gB)).norm()), float(gA.norm()) + float(gB.norm())
    print(f"window gradient vs gA + gB: {err:.3e} of {scale:.3e} ({err / scale:.2e})")
    assert scale > 0 and err <= 8e-6 * scale, (err, scale)


def test_exchange_schedule_at_world_one(tmp_path):
    out = str(tmp_path / "accum.pt")
    port = str(31000 + os.getpid() % 2000)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.Popen([sys.executable, "-m", "tests.accum_worker", port, out], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True)
    try:
        log, _ = p.communicate(timeout=300)
    except subprocess.TimeoutExpired:
        p.kill()
        raise
    assert p.returncode == 0, log[-4000:]
    r = torch.load(out, weights_only=False)
    # one collective per gradient bucket per window, last segment first, whole slices -- and none on a window's first micro-batch
    per_window = list(reversed(r["bucket_elems"]))
    assert r["per_micro_batch"] == [[], per_window, [], per_window], r["per_micro_batch"]
    assert all(math.isfinite(l) for l in r["losses"]) and len(r["losses"]) == 4
    assert not same(r["alone"], r["ranked"]), same(r["alone"], r["ranked"])
    assert r["ranked"]["host_step"] == r["alone"]["host_step"] and torch.isfinite(r["ranked"]["flat_p"]).all()


def test_speechbrain_env_updates_once_per_window(tmp_path):
    from fqss_amd import checkpoint
    from fqss_amd.train_env.speechbrain_librimix import speechbrain_librimix_trainer as T
    text = open(os.path.join(ROOT, "configs", "sepformer_2spks_8k_synthetic.yaml")).read()
    text = text.replace("training_signal_len: 32000", "training_signal_len: 4000").replace("steps_per_epoch: 60", "steps_per_epoch: 5")
    text = text.replace("val_steps: 4", "val_steps: 1")
    steps = {}
    for name, extra in (("accum", "grad_accumulation_factor: 2\n"), ("plain", "")):
        work = tmp_path / name
        yml = tmp_path / f"{name}.yaml"
        yml.write_text(text.replace("work_dir: /tmp/fqss_sepformer_synth", f"work_dir: {work}") + extra)
        assert T.load_hparams(str(yml)).get("grad_accumulation_factor") == (2 if extra else None)
        hist = T.train(str(yml), 0, False, "cuda")
        assert len(hist) == 2 and all(math.isfinite(h["train_loss"]) for h in hist), hist
        ck = checkpoint.load_training_state(os.path.join(str(work), "checkpoint.pth"))
        steps[name] = (ck["step"]["arena"]["host_step"], int(ck["step"]["arena"]["step_t"]))
    # five micro-batches per epoch in windows of two: two full windows and one flushed, in each of the two epochs
    assert steps == {"accum": (6, 6), "plain": (10, 10)}, steps


def test_htdemucs_env_updates_once_per_window(tmp_path, monkeypatch):
    import yaml
    from fqss_amd import checkpoint
    from fqss_amd.train_env.htdemucs_musdbhq import train as T
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "htdemucs_synthetic.yaml")))
    conf["work_dir"] = str(tmp_path / "run")
    conf["dset"].update(segment=0.05, sources=["a", "b"], steps_per_epoch=3, valid_steps=1)
    conf.update(epochs=1, batch_size=2, weights=[1.0, 1.0])
    conf["htdemucs"] = dict(nfft=2048, channels=8, bottom_channels=16, t_layers=3, t_heads=2)
    yml = tmp_path / "cfg.yaml"
    yml.write_text(yaml.safe_dump(conf))
    monkeypatch.setattr(sys, "argv", ["train.py", "+device=cuda", f"+yml_path={yml}", "+optim.accumulate_grad_batches=2"])
    hist = T.main()
    assert len(hist) == 1 and math.isfinite(hist[0]["train"]["loss"]) and math.isfinite(hist[0]["valid"]["loss"])
    ck = checkpoint.load_training_state(os.path.join(conf["work_dir"], "checkpoint.pth"))
    # three micro-batches in windows of two: one full window and one flushed
    assert ck["step"]["arena"]["host_step"] == 2 and int(ck["step"]["arena"]["step_t"]) == 2
