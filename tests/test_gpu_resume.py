"""GPU: resuming an interrupted QAT run from the full training-state checkpoint (fqss_amd/checkpoint.py).

  B. asteroid env, full ConvTasNet, FQSS_DETERMINISTIC=1: a run stopped after epoch 1 (inside the observer phase) or after epoch 2
     (on replayed graphs) and resumed ends bit-identical to the uninterrupted run;
  C. stepper level, the tiny model of every family with its own loss: state_dict() -> new objects -> load_state_dict() keeps every
     tensor and flag, the next step computes what the uninterrupted stepper computes, and the resumed stepper leaves the observer
     phase, captures and replays;
  D. two ranks (gloo, tests/resume_ddp_worker.py): a file written before the range synchronisation gives every rank its own ranges
     back and refuses another world size;
  E. the speechbrain and htdemucs trainers: stop after epoch 1, resume, end with the full history and the restored best / scheduler."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- B: the asteroid trainer -----------------------------------------------------------------------------------------------------
def _asteroid(tmp_path, name, epochs, resume=None):
    from fqss_amd.train_env.asteroid_librimix import asteroid_librimix_trainer as A
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "convtasnet_2spks_8k_synthetic.yaml")))
    conf["work_dir"] = str(tmp_path / name)
    # validation forwards count as observer calls too: epoch 1 ends at n_iter 28 (observer phase), the phase ends inside epoch 2,
    # which finishes on replayed graphs, epoch 3 is all quantizing
    conf["dataset_cfg"].update(segment=0.25, steps_per_epoch=26, val_steps=2)
    conf["training_cfg"].update(epochs=epochs, batch_size=2)
    if resume is not None:
        conf["training_cfg"]["resume"] = resume
    yml = tmp_path / f"{name}_{epochs}.yaml"
    yml.write_text(yaml.safe_dump(conf))
    t = time.perf_counter()
    hist = A.train(str(yml), "cuda")
    print(f"asteroid run {name}: epochs -> {epochs}, resume={resume}: {time.perf_counter() - t:.1f} s")
    return hist, conf["work_dir"]


def test_asteroid_run_resumed_after_epoch_1_or_2_is_bit_identical_to_the_uninterrupted_run(tmp_path, monkeypatch):
    """relies on FQSS_DETERMINISTIC=1 making identical streams bit-equal and on an eager step and a replayed step producing the same
    bits (tests/test_gpu_kdstep_path.py): the run resumed after epoch 2 takes one eager step where the uninterrupted run replays"""
    from fqss_amd import checkpoint
    monkeypatch.setenv("FQSS_DETERMINISTIC", "1")
    hist_u, dir_u = _asteroid(tmp_path, "u", 3)
    assert [h["launch"] for h in hist_u] == ["eager", "hipGraph replay", "hipGraph replay"]
    want = torch.load(os.path.join(dir_u, "latest_model.pth"), weights_only=True)
    assert len(want) == 948
    for stop in (1, 2):
        name = f"stop{stop}"
        hist_s, dir_s = _asteroid(tmp_path, name, stop)
        ck = checkpoint.load_training_state(os.path.join(dir_s, "checkpoint.pth"))
        n_iter = {q["n_iter"] for q in ck["step"]["act_quantizers"].values()}
        assert ck["trainer"]["epoch"] == stop and min(n_iter) == (28 if stop == 1 else 50) and max(n_iter) <= 50, n_iter
        hist_r, _ = _asteroid(tmp_path, name, 3, resume="auto")
        assert [h["epoch"] for h in hist_r] == [0, 1, 2] and hist_r[:stop] == hist_s
        for hu, hr in zip(hist_u, hist_r):
            for k in ("loss", "val_loss", "lr"):
                assert hu[k] == hr[k], (stop, k, hu, hr)
        got = torch.load(os.path.join(dir_s, "latest_model.pth"), weights_only=True)
        differ = [k for k in want if not torch.equal(want[k], got[k])]
        assert list(got) == list(want) and not differ, (stop, len(differ), differ[:5])
        ck_u, ck_r = (checkpoint.load_training_state(os.path.join(d, "checkpoint.pth")) for d in (dir_u, dir_s))
        for k in ("exp_avg", "exp_avg_sq", "t0", "step_t"):
            assert torch.equal(ck_u["step"]["arena"][k], ck_r["step"]["arena"][k]), (stop, k)


# ---- C: the stepper, every family ------------------------------------------------------------------------------------------------
OBS = 4         # observer calls of the stepper tests (the modules' max_observations; 50 in training): the phase positions are what count


def _family(name, g):
    """-> (build() -> (model, fmodel), x, tgt, KDTrainStep keywords): the tiny pairs of the existing GPU tests from their fixtures' initial
    state, each with its environment's loss"""
    if name == "convtasnet":
        from tests.test_gpu_model import _tiny_pair
        return (lambda: _tiny_pair(g)), T(g["x"]).cuda(), T(g["tgt"]).cuda(), dict(kd_lambda=0.1, lr=1e-3, clip=5.0)
    if name == "dptnet":
        from tests.test_gpu_dptnet import _tiny_pair
        return (lambda: _tiny_pair(g)), T(g["x"]).cuda(), T(g["tgt"]).cuda(), dict(kd_lambda=0.1, lr=4e-4, clip=5.0)
    if name == "sepformer":
        from tests.test_gpu_sepformer import _tiny_pair
        kw = dict(kd_lambda=0.1, lr=1.5e-4, clip=5.0, loss="sisdr_pit_per_sample", loss_threshold=-30.0)
        return (lambda: _tiny_pair(g)), T(g["x"]).cuda(), T(g["tgt"]).cuda(), kw
    from tests.test_gpu_htdemucs import _models
    return (lambda: _models(g)), T(g["mix"]).cuda(), T(g["src"]).cuda(), dict(kd_lambda=0.1, lr=3e-4, clip=0.0, loss="l1_sdr")


FIXTURE = dict(convtasnet="tiny_step", dptnet="dpt_tiny_step", sepformer="sep_tiny_step", htdemucs="hd_tiny_step")


def _same(a, b, path="state"):
    """two state trees equal bit for bit: same keys, same plain values, torch.equal tensors of the same dtype"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for k in a:
            _same(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (u, v) in enumerate(zip(a, b)):
            _same(u, v, f"{path}[{i}]")
    elif torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape, path
        assert torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8)), path
    else:
        assert type(a) is type(b) and a == b, (path, a, b)


@pytest.mark.parametrize("fam", ["convtasnet", "dptnet", "sepformer", "htdemucs"])
def test_stepper_state_round_trip_and_next_step(golden, fam, monkeypatch, capsys):
    """Round trip and next step at two points: N1 = 2 (inside the observer phase) and N2 = OBS + 3 (after the capture: OBS observer
    steps, one eager quantizing step, two replays).  "The same" at step N + 1 is what two fresh steppers without any checkpoint give:
    where they agree bit for bit the resumed step must too, otherwise twice their difference is allowed.  Measured on an MI355X
    (|loss|, max |est|): ConvTasNet and HTDemucs 0 / 0 at both points; DPTNet 0 / 1.2e-7 at N1 and 9.4e-3 / 1.6e-2 at N2; Sepformer
    0 / 0 at N1 and 1.5e-1 / 2.8e-2 at N2 (their backward is not bit-reproducible, and seven steps amplify it).  The resumed step
    differed from the uninterrupted stepper's by 0 / 0 in every family at both points: loss and output of step N + 1 are a forward pass
    over the restored state, and the forward is deterministic."""
    from fqss_amd.quantization.qat.qat_quant import GradientActivationFakeQuantize
    from fqss_amd.runtime import KDTrainStep
    monkeypatch.setenv("FQSS_DETERMINISTIC", "1")
    build, x, tgt, kw = _family(fam, golden(FIXTURE[fam]))
    N1, N2 = 2, OBS + 3

    def fresh():
        model, fmodel = build()
        for m in model.modules():
            if isinstance(m, GradientActivationFakeQuantize):
                m.max_observations = OBS
        return KDTrainStep(model, fmodel, **kw)

    def one(step):
        step.maybe_capture(x, tgt)
        r = step(x, tgt)
        return r["loss"].detach().clone(), r["est"].detach().clone()

    # the uninterrupted stepper: snapshots behind steps N1 and N2, results of steps N1 + 1 and N2 + 1
    a, snap, res_a = fresh(), {}, {}
    for s in range(1, N2 + 2):
        res_a[s] = one(a)
        if s in (N1, N2):
            snap[s] = a.state_dict()
            assert (a._graphs is not None) == (s == N2) and a.can_capture() == (s == N2)
    # the yardstick: two fresh steppers, no checkpoint involved
    res_f = []
    for _ in range(2):
        f, rf = fresh(), {}
        for s in range(1, N2 + 2):
            rf[s] = one(f)
        res_f.append(rf)
        del f
    for n in (N1, N2):
        b = fresh()
        with torch.no_grad():                   # nothing of the fresh initialisation may survive the load
            b.arena.flat_p.add_(0.01)
            b.arena.exp_avg.fill_(1.0)
        p_ptrs = [p.data_ptr() for p in b.arena.params]
        b.load_state_dict(snap[n])
        assert [p.data_ptr() for p in b.arena.params] == p_ptrs
        _same(snap[n], b.state_dict())
        assert (b.tables, b._graphs, b._tgraph, b._ahead, b._eager_q) == (None, None, None, None, 0)
        assert b.arena._host_step == n and len(b.arena._inactive) == len([1 for p, o in zip(b.arena.params, b.arena.offsets)
                                                                            if int(b.arena.t0[o]) == 2 ** 31 - 1])
        loss_b, est_b = one(b)
        assert b._graphs is None                # the step behind a load runs eagerly (it rebuilds the tables)
        d_loss = float((res_f[0][n + 1][0] - res_f[1][n + 1][0]).abs())
        d_est = float((res_f[0][n + 1][1] - res_f[1][n + 1][1]).abs().max())
        e_loss, e_est = float((loss_b - res_a[n + 1][0]).abs()), float((est_b - res_a[n + 1][1]).abs().max())
        with capsys.disabled():
            print(f"\n[resume {fam} N={n}] fresh-vs-fresh: loss {d_loss:.3e} est {d_est:.3e}; resumed-vs-uninterrupted: loss {e_loss:.3e} est {e_est:.3e}")
        assert torch.isfinite(loss_b) and e_loss <= 2 * d_loss and e_est <= 2 * d_est, (fam, n, e_loss, d_loss, e_est, d_est)
        # on from there: out of the observer phase, one eager quantizing step, capture, three replays
        for _ in range(OBS + 1 - (n + 1) if n == N1 else 0):
            one(b)
        assert b.can_capture() and b._eager_q >= 1 and b.tables is not None
        for _ in range(3):
            loss, _ = one(b)
            assert b._graphs is not None and torch.isfinite(loss)
        del b


# ---- D: two ranks ----------------------------------------------------------------------------------------------------------------
def test_two_ranks_resume_with_their_own_observer_ranges(tmp_path):
    port = str(31000 + (os.getpid() * 7) % 2000)
    outs = [str(tmp_path / f"rank{r}.pt") for r in range(2)]
    ckpt = str(tmp_path / "checkpoint.pth")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    ps = [subprocess.Popen([sys.executable, "-m", "tests.resume_ddp_worker", str(r), "2", port, outs[r], ckpt], cwd=ROOT, env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = []
    for p in ps:
        try:
            out, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in ps:
                q.kill()
            raise
        logs.append(out)
    assert all(p.returncode == 0 for p in ps), "\n----\n".join(logs)
    r0, r1 = (torch.load(o, weights_only=False) for o in outs)
    for r in (r0, r1):
        # what each rank held when the file was written is what it holds after the resume, n_iter included; still unsynchronised
        assert r["n_iter_loaded"] == r["n_iter_saved"] and 0 < r["n_iter_saved"] < 50 and r["synced_loaded"] is False
        assert set(r["loaded"]) == set(r["saved"]) and all(torch.equal(r["loaded"][k], v) for k, v in r["saved"].items())
        assert r["synced_end"] is True and all(torch.isfinite(torch.tensor(r["losses"])))
    assert any(not torch.equal(r0["saved"][k], r1["saved"][k]) for k in r0["saved"])         # the shards differ, so do the ranges
    assert all(torch.equal(r0["end"][k], r1["end"][k]) for k in r0["end"])                    # ... until the phase ends
    # the same file at world 1
    from fqss_amd import checkpoint
    from fqss_amd.runtime import KDTrainStep
    from tests.test_gpu_model import _tiny_pair
    g = np.load(os.path.join(ROOT, "tests", "golden", "tiny_step.npz"))
    ck = checkpoint.load_training_state(ckpt)
    assert ck["step"]["world"] == 2 and tuple(ck["step"]["rank_ranges"].shape)[::2] == (2, 3)
    step = KDTrainStep(*_tiny_pair(g), kd_lambda=0.1, lr=1e-3, clip=5.0)
    with pytest.raises(ValueError, match="world size 2"):
        checkpoint.restore(ck, step, step.fmodel)


# ---- E: the other two trainers ---------------------------------------------------------------------------------------------------
def test_speechbrain_env_resumes_after_epoch_1(tmp_path):
    """the sizes of tests/test_gpu_env.py.  The stored `best` and scheduler fields are what the resumed epoch works with: the file is
    edited between the two calls (best below anything reachable, the scheduler one bad epoch from halving), so epoch 2 must leave
    best_model.pth alone and must halve the learning rate"""
    from fqss_amd import checkpoint
    from fqss_amd.train_env.speechbrain_librimix import speechbrain_librimix_trainer as S
    text = open(os.path.join(ROOT, "configs", "sepformer_2spks_8k_synthetic.yaml")).read()
    text = text.replace("work_dir: /tmp/fqss_sepformer_synth", f"work_dir: {tmp_path / 'run'}")
    text = text.replace("training_signal_len: 32000", "training_signal_len: 4000").replace("steps_per_epoch: 60", "steps_per_epoch: 3")
    text = text.replace("val_steps: 4", "val_steps: 1")
    assert "N_epochs: 2" in text and "dont_halve_until_epoch: 20" in text and "patience: 3" in text and "factor: 0.5" in text
    text = text.replace("dont_halve_until_epoch: 20", "dont_halve_until_epoch: 1")      # the scheduler may act from epoch 2 on
    one = tmp_path / "one.yaml"
    one.write_text(text.replace("N_epochs: 2", "N_epochs: 1"))
    two = tmp_path / "two.yaml"
    two.write_text(text + "\nresume: auto\n")
    hist1 = S.train(str(one), 0, False, "cuda")
    save = tmp_path / "run" / "save"
    state = tmp_path / "run" / "checkpoint.pth"
    assert len(hist1) == 1 and hist1[0]["epoch"] == 1 and state.exists() and not (save / "checkpoint.pth").exists()
    best_bytes = (save / "best_model.pth").read_bytes()
    ck = checkpoint.load_training_state(str(state))
    assert ck["trainer"]["epoch"] == 1 and ck["trainer"]["best"] == hist1[0]["valid_si-snr"] and ck["trainer"]["sched"]["losses"] == [hist1[0]["valid_si-snr"]]
    lr = ck["step"]["lr"]
    ck["trainer"]["best"] = -1e9
    ck["trainer"]["sched"].update(anchor=-1e9, patience_counter=3)
    checkpoint.write_atomic(ck, str(state))
    hist2 = S.train(str(two), 0, False, "cuda")
    assert [h["epoch"] for h in hist2] == [1, 2] and hist2[0] == hist1[0] and np.isfinite(hist2[1]["train_loss"])
    assert (save / "best_model.pth").read_bytes() == best_bytes                      # best = -1e9 came from the file
    assert (save / "latest_model.pth").read_bytes() != best_bytes
    end = checkpoint.load_training_state(str(state))
    assert end["trainer"]["epoch"] == 2 and end["trainer"]["best"] == -1e9 and len(end["trainer"]["sched"]["losses"]) == 2
    assert hist2[1]["lr"] == lr and end["step"]["lr"] == lr * 0.5   # the restored scheduler halved
    assert S.train(str(two), 0, False, "cuda") == hist2                               # finished: the stored history, nothing else


def test_htdemucs_env_resumes_after_epoch_1(tmp_path, monkeypatch):
    """the sizes of tests/test_gpu_env.py; the observer phase ends inside the resumed epoch 2.  The stored best_loss (edited to lie below
    anything reachable) and best_state are what the resumed solver keeps: best.th still holds epoch 1's state after a worse epoch 2"""
    from fqss_amd import checkpoint
    from fqss_amd.train_env.htdemucs_musdbhq import train as H
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "htdemucs_synthetic.yaml")))
    conf["work_dir"] = str(tmp_path / "run")
    conf["dset"].update(segment=0.05, sources=["a", "b"], steps_per_epoch=28, valid_steps=1)
    conf.update(epochs=2, batch_size=2, weights=[1.0, 1.0])
    conf["htdemucs"] = dict(nfft=2048, channels=8, bottom_channels=16, t_layers=3, t_heads=2)
    yml = tmp_path / "cfg.yaml"
    yml.write_text(yaml.safe_dump(conf))
    monkeypatch.setattr(sys, "argv", ["train.py", "+device=cuda", f"+yml_path={yml}", "optim.lr=0.0002", "epochs=1"])
    hist1 = H.main()
    assert len(hist1) == 1 and hist1[0]["train"]["launch"] == "eager"
    path = os.path.join(conf["work_dir"], "checkpoint.pth")
    best1 = torch.load(os.path.join(conf["work_dir"], "best.th"), weights_only=True)["state"]
    ck = checkpoint.load_training_state(path)
    assert ck["trainer"]["epoch"] == 1 and ck["trainer"]["best_loss"] == hist1[0]["valid"]["loss"]
    assert all(torch.equal(v, ck["trainer"]["best_state"][k]) for k, v in best1.items())
    ck["trainer"]["best_loss"] = -1e9
    checkpoint.write_atomic(ck, path)
    monkeypatch.setattr(sys, "argv", ["train.py", "+device=cuda", f"+yml_path={yml}", "optim.lr=0.0002", "+resume=auto"])
    hist2 = H.main()
    assert len(hist2) == 2 and hist2[0] == hist1[0] and np.isfinite(hist2[1]["train"]["loss"]) and np.isfinite(hist2[1]["valid"]["loss"])
    assert hist2[1]["train"]["launch"] == "hipGraph replay" and hist2[1]["valid"]["best"] == -1e9
    pkg = torch.load(os.path.join(conf["work_dir"], "best.th"), weights_only=True)
    assert len(pkg["history"]) == 2 and all(torch.equal(v, pkg["state"][k]) for k, v in best1.items())
    assert H.main() == hist2                                                          # finished: the stored history, nothing else
