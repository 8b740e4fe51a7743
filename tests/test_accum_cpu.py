"""Gradient accumulation, without a GPU: fqss_grad_accum of the CPU backend bit for bit against torch, and the window arithmetic of
KDTrainStep(accumulate=N) against the same two micro-batches summed by hand -- the CPU backend is bit-reproducible, so equality is
the bar.  A window of N micro-batches takes one clip + Adam update on the SUM of their gradients at grad_scale 1 / (world * N)."""
import os
import subprocess

import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.0
STATE = ("flat_p", "exp_avg", "exp_avg_sq", "step_t", "t0", "gnorm")


@pytest.fixture()
def cpu_backend():
    from fqss_amd import _lib
    if not os.path.exists(_lib.CPU_SO_PATH):
        subprocess.check_call(["make", "-C", os.path.dirname(_lib.CPU_SO_PATH)])
    prev = _lib.BACKEND
    _lib.set_backend("cpu")
    yield
    _lib.set_backend(prev)


# ---- 1. the kernel --------------------------------------------------------------------------------------------------------------
def check_grad_accum(device):
    """shared with tests/test_gpu_accum.py: all four modes, whole buffers and a slice between sentinels, the refused arguments"""
    from fqss_amd import _lib
    from fqss_amd import kernels as K
    g = torch.Generator().manual_seed(0)
    cases = [(n, 0, n) for n in (64, 64 * 5, 64 * 33)] + [(64 * 9, 64 * 2, 64 * 7)]
    for total, lo, hi in cases:
        for mode in range(4):
            acc0, g0 = torch.randn(total, generator=g).to(device), torch.randn(total, generator=g).to(device)
            acc, gr = acc0.clone(), g0.clone()
            if (lo, hi) != (0, total):
                for t in (acc, gr):
                    t[:lo] = SENTINEL
                    t[hi:] = SENTINEL
            K.grad_accum(acc[lo:hi], gr[lo:hi], mode)
            a, b = acc0[lo:hi], g0[lo:hi]
            want_acc, want_g = {0: (b, b), 1: (a + b, b), 2: (a, a + b), 3: (a, a)}[mode]
            assert torch.equal(acc[lo:hi], want_acc) and torch.equal(gr[lo:hi], want_g), (total, lo, hi, mode)
            if (lo, hi) != (0, total):
                for t in (acc, gr):
                    assert (t[:lo] == SENTINEL).all() and (t[hi:] == SENTINEL).all(), (mode, "wrote outside the slice")
    buf, oth = torch.zeros(256, device=device), torch.zeros(256, device=device)
    with pytest.raises(_lib.FqssError):
        K.grad_accum(buf[:66], oth[:66], 1)                       # n = 66
    with pytest.raises(_lib.FqssError):
        K.grad_accum(buf[1:65], oth[0:64], 1)                     # a base one float off 16 bytes
    with pytest.raises(_lib.FqssError):
        K.grad_accum(buf[:64], oth[:64], 4)                       # no such mode
    with pytest.raises(_lib.FqssError):
        _lib.call("fqss_grad_accum", None, oth.data_ptr(), 64, 1, K._stream())
    _lib.call("fqss_grad_accum", buf.data_ptr(), oth.data_ptr(), 0, 1, K._stream())      # n = 0: nothing to do
    K.grad_accum(buf[:0], oth[:0], 1)
    assert not buf.any() and not oth.any()


def test_grad_accum_equals_torch_bit_for_bit(cpu_backend):
    check_grad_accum("cpu")


# ---- 2.-5. the window -------------------------------------------------------------------------------------------------------------
TINY4 = dict(n_spks=2, kernel_size=16, stride=8, n_filters=32, bn_chan=16, hid_chan=32, n_blocks=4, n_repeats=1)


def make_step(device, kw, **step_kw):
    from fqss_amd.runtime import KDTrainStep
    from fqss_amd.smoke import build_pair
    model, fmodel = build_pair(device, 0, **kw)
    return KDTrainStep(model, fmodel, kd_lambda=0.1, lr=1e-3, clip=5.0, **step_kw)


def settle(step, device):
    """leave the observer phase: one observing call, n_iter = max_observations, one quantizing call (the weight observers run)"""
    from fqss_amd.data import synth_batch
    from fqss_amd.quantization.qat import qat_quant as QQ
    x, tgt = synth_batch(2, 4000, seed=7, device=device)
    step(x, tgt)
    for m in step.model.modules():
        if isinstance(m, QQ.GradientActivationFakeQuantize):
            m.n_iter = m.max_observations
    step(x, tgt)
    assert step.can_capture()
    return step


def snapshot(step):
    a = step.arena
    return {k: getattr(a, k).clone() for k in STATE} | {"host_step": a._host_step}


def same(u, v, keys=STATE + ("host_step",)):
    return [k for k in keys if not (torch.equal(u[k], v[k]) if torch.is_tensor(u[k]) else u[k] == v[k])]


def pair_of_steps(device, kw, **step_kw):
    """(reference step without accumulation, step under test), identically seeded and in ONE state past the observer phase: the
    reference is taken there and its whole training state -- parameters, moments, clocks, quantizer flags -- loaded into both (a load
    drops the quantizer tables, so both rebuild them on their next call)"""
    ref = settle(make_step(device, kw), device)
    got = make_step(device, kw, **step_kw)
    sd = ref.state_dict()
    got.load_state_dict(sd)
    ref.load_state_dict(sd)
    assert not same(snapshot(ref), snapshot(got), STATE[:-1] + ("host_step",)) and got.can_capture()
    return ref, got


def reference_window(ref, grads, batches):
    """the issue's reference: the micro-batch gradients summed in torch, one activation, one clip + Adam at grad_scale 1 / 2"""
    a = ref.arena
    total = None
    for i, (x, tgt) in enumerate(batches):
        ref._step_eager(x, tgt)
        if grads[i]:
            total = a.flat_g.clone() if total is None else total + a.flat_g
    a.flat_g.copy_(total)
    a._activate_touched()
    a.clip_adam_step(ref.lr, ref.clip, grad_scale=0.5, activate=False)
    return snapshot(ref)


def ab(device):
    from fqss_amd.data import synth_batch
    return synth_batch(2, 4000, seed=0, device=device), synth_batch(2, 4000, seed=1, device=device)


def test_window_of_two_equals_the_summed_gradients(cpu_backend):
    A, B = ab("cpu")
    ref, got = pair_of_steps("cpu", TINY4, accumulate=2)
    before = snapshot(got)
    want = reference_window(ref, (True, True), (A, B))
    r = got(*A)
    assert set(r) == {"loss", "kd_loss", "task", "kd", "w", "sisdr", "gnorm", "est"}
    after_a = snapshot(got)
    assert not same(before, after_a, ("flat_p", "exp_avg", "exp_avg_sq", "step_t", "t0", "host_step")) and got.pending == 1
    got(*B)
    assert got.pending == 0
    assert not same(want, snapshot(got)), same(want, snapshot(got))
    assert not torch.equal(want["flat_p"], before["flat_p"]) and int(want["step_t"]) == int(before["step_t"]) + 1


def test_flush_updates_on_what_the_window_holds(cpu_backend):
    A, B = ab("cpu")
    ref, got = pair_of_steps("cpu", TINY4, accumulate=2)
    assert got.flush() is False                                   # nothing pending: nothing happens
    want = reference_window(ref, (True,), (A,))
    got(*A)
    with pytest.raises(RuntimeError, match="pending"):
        got.state_dict()
    assert got.flush() is True and got.pending == 0
    assert not same(want, snapshot(got)), same(want, snapshot(got))
    assert got.flush() is False
    assert not same(want, snapshot(got))
    assert got.state_dict()["arena"]["host_step"] == want["host_step"]


def test_commit_keep_false_drops_a_micro_batch(cpu_backend):
    A, B = ab("cpu")
    ref, got = pair_of_steps("cpu", TINY4, accumulate=2)
    want = reference_window(ref, (True, False), (A, B))           # (the reference runs B too: its forward moves no state that matters)
    got.micro_batch(*A)
    assert got.commit(True) is False
    got.micro_batch(*B)
    assert got.commit(False) is True and got.pending == 0
    assert not same(want, snapshot(got)), same(want, snapshot(got))
    # a window in which everything was dropped: no update, no clock
    before = snapshot(got)
    for batch in (A, B):
        got.micro_batch(*batch)
        assert got.commit(False) is False
    assert got.pending == 0
    assert not same(before, snapshot(got), ("flat_p", "exp_avg", "exp_avg_sq", "step_t", "t0", "host_step"))
    with pytest.raises(RuntimeError):
        got.commit()                                              # nothing to commit


def test_accumulate_one_is_the_step_as_it_was(cpu_backend):
    A, B = ab("cpu")
    plain, one = make_step("cpu", TINY4), make_step("cpu", TINY4, accumulate=1)
    assert one.arena.acc is None and plain.arena.acc is None and make_step("cpu", TINY4, accumulate=2).arena.acc is not None
    for batch in (A, B, A):
        plain(*batch)
        one(*batch)
        assert one.pending == 0
    assert not same(snapshot(plain), snapshot(one)), same(snapshot(plain), snapshot(one))
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError):
            make_step("cpu", TINY4, accumulate=bad)


# ---- 6. the asteroid env ----------------------------------------------------------------------------------------------------------
def test_asteroid_env_on_the_cpu_backend_counts_updates_per_window(tmp_path, cpu_backend, monkeypatch):
    """the trainer's loop, its flush at the end of an epoch and the Adam clocks in the checkpoint.  What is counted does not depend on
    the network's size, so the trainer builds the four-block ConvTasNet of the tests above instead of the config's 5.1 M parameter
    one (24 CPU steps of that take a minute and a half); every key of the config is read as in any run"""
    import math
    from fqss_amd import checkpoint
    from fqss_amd.smoke import build_pair
    from fqss_amd.train_env.asteroid_librimix import asteroid_librimix_trainer as T
    monkeypatch.setattr(T, "create_pretrained_model", lambda model_cfg: build_pair("cpu", 0, **TINY4))
    steps = {}
    for name, n in (("accum", 2), ("plain", None)):
        cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "convtasnet_2spks_8k_cpu.yaml")))
        cfg["work_dir"] = str(tmp_path / name)
        cfg["dataset_cfg"].update(steps_per_epoch=5, val_steps=1)
        cfg["training_cfg"].update(epochs=2)
        if n is not None:
            cfg["training_cfg"]["accumulate_grad_batches"] = n
        yml = tmp_path / f"{name}.yaml"
        yml.write_text(yaml.safe_dump(cfg))
        hist = T.train(str(yml), "cpu")
        assert len(hist) == 2 and all(math.isfinite(h["loss"]) and math.isfinite(h["val_loss"]) for h in hist), hist
        ck = checkpoint.load_training_state(os.path.join(cfg["work_dir"], "checkpoint.pth"))
        steps[name] = (ck["step"]["arena"]["host_step"], int(ck["step"]["arena"]["step_t"]))
    # five micro-batches per epoch in windows of two: two full windows and one flushed
    assert steps == {"accum": (6, 6), "plain": (10, 10)}, steps
