"""`train(yml_path, device)` of the asteroid env (reference: asteroid_librimix_trainer.py:140-214),
MI355X edition: same YAML keys (work_dir, model_cfg{,.quantization}, dataset_cfg, training_cfg), same
outputs (conf.yml, latest_model.pth, best_model.pth = student state_dict), data-parallel over the
GPUs of one node when launched with torch.distributed.run (one process per GPU, RCCL).  Every epoch also ends with
`<work_dir>/checkpoint.pth`, the full training state; `training_cfg.resume: <path> | auto` continues from one (fqss_amd/checkpoint.py).

Data: `dataset_cfg.name: librimix` is the reference's own configuration (configs/convtasnet_2spks_8k.yaml:27-41): `prepare_datasets`
builds the LibriMix CSV datasets exactly as asteroid_librimix_trainer.py:26-75 does and feeds them through a background reader
(fqss_amd/loader.py: WAV reads, upload, resampling and SNR mixing of batch n+1 on a side stream while step n replays).
`dataset_cfg.name: synthetic` generates the seeded 2-speaker mixtures of the measurement contract."""
import json
import os

import torch
import yaml

from ... import checkpoint
from ...data import synth_batch
from ...loader import Prefetcher, epoch_batches, with_lookahead
from ...parallel import Comm
from ...utils import set_seed
from ..train_utils import create_pretrained_model
from .mysystem import System


LAST_SYSTEM = None


def prepare_datasets(dataset_cfg, training_cfg, device):
    """train / validation LibriMix sets with the reference's arguments (asteroid_librimix_trainer.py:26-52)"""
    from .librimix_dataset import LibriMix
    augmentation_cfg = dataset_cfg.get("augmentation", None)
    if augmentation_cfg and not augmentation_cfg.get("enable", False):
        augmentation_cfg = None
    common = dict(task=dataset_cfg["task"], sample_rate=dataset_cfg["sample_rate"], resample=dataset_cfg.get("resample", 1),
                  n_src=dataset_cfg["n_src"], segment=dataset_cfg["segment"], device=device)
    train_set = LibriMix(csv_dir=dataset_cfg["train_dir"], augmentation_cfg=augmentation_cfg, **common)
    val_set = LibriMix(csv_dir=dataset_cfg["valid_dir"], **common)
    print("Training set size: {}".format(len(train_set)))
    print("Validation set size: {}".format(len(val_set)))
    return train_set, val_set


class _Data:
    """the two loaders of prepare_datasets (:53-67): shuffled / sequential batches of training_cfg.batch_size, drop_last; under DDP
    every rank reads its DistributedSampler share (Lightning's replacement sampler).  `train(epoch)` yields (x, tgt, x_next)."""

    def __init__(self, dataset_cfg, training_cfg, comm, device, n_src=2):
        self.cfg, self.tc, self.comm, self.device, self.n_src = dataset_cfg, training_cfg, comm, device, int(n_src)
        self.synthetic = dataset_cfg.get("name") == "synthetic"
        self.loader_wait_s = 0.0
        if self.synthetic:
            return
        if dataset_cfg.get("name") != "librimix":
            raise NotImplementedError(f"asteroid env: dataset_cfg.name {dataset_cfg.get('name')!r} (librimix | synthetic)")
        self.train_set, self.val_set = prepare_datasets(dataset_cfg, training_cfg, device)

    def _synthetic(self, split):
        ds, comm = self.cfg, self.comm
        sr = int(ds.get("sample_rate", 16000) * ds.get("resample", 0.5))
        T = int(ds.get("segment", 3) * sr)
        n = int(ds.get("steps_per_epoch" if split == "train" else "val_steps", 20 if split == "train" else 4))
        for i in range(n):
            yield synth_batch(self.tc["batch_size"], T, seed=(0 if split == "train" else 10_000) + i * comm.world + comm.rank,
                              device=self.device, n_src=self.n_src)

    def _files(self, split, epoch):
        ds = self.train_set if split == "train" else self.val_set
        batches = epoch_batches(len(ds), self.tc["batch_size"], shuffle=split == "train", drop_last=True, rank=self.comm.rank,
                                world=self.comm.world, seed=self.tc.get("seed", 0), epoch=epoch)
        limit = self.cfg.get("steps_per_epoch" if split == "train" else "val_steps")      # optional cap (smoke runs), not a reference key
        if limit is not None:
            batches = batches[:int(limit)]
        pf = Prefetcher(ds, batches, self.device, depth=int(self.tc.get("prefetch_depth", 2)))
        yield from pf
        self.loader_wait_s += pf.wait_s

    def train(self, epoch):
        return with_lookahead(self._synthetic("train") if self.synthetic else self._files("train", epoch))

    def val(self, epoch):
        return self._synthetic("val") if self.synthetic else self._files("val", epoch)


def train(yml_path, device, resume=None):
    """resume: a training-state checkpoint to continue from, or "auto" (`--resume` of fqss_amd.train); overrides `training_cfg.resume`"""
    from ... import _lib
    prev = _lib.BACKEND
    try:
        return _train(yml_path, device, resume)
    finally:
        if _lib.BACKEND != prev:          # `--use_cpu` switched the process to the CPU backend: hand it back as it was found
            _lib.set_backend(prev)


def _train(yml_path, device, resume=None):
    cpu = device == "cpu"
    if cpu:
        # `--use_cpu` (reference train.py:31; BASELINE.json configs[0]: "CPU, batch 2, 1 s ... plumbing, no GPU"): the same trainer over
        # the CPU backend of the C ABI (csrc/cpu/libfqss_cpu.so: the un-fused per-layer entry points of the ConvTasNet step).  Chosen
        # explicitly here, never as a fallback; oracle/ is not involved.
        from ... import _lib
        _lib.set_backend("cpu")
    with open(yml_path) as f:
        conf = yaml.safe_load(f)
    work_dir, model_cfg, dataset_cfg = conf["work_dir"], conf["model_cfg"], conf["dataset_cfg"]
    training_cfg = conf["training_cfg"]
    set_seed(training_cfg.get("seed", 0))
    comm = Comm.from_env("cpu" if cpu else "cuda")
    # `training_cfg.resume: <path> | auto`: continue from the full training state an earlier launch left (fqss_amd/checkpoint.py)
    if resume is not None:
        training_cfg["resume"] = resume
    ckpt = checkpoint.resume_path(training_cfg.get("resume"), work_dir)
    ckpt = checkpoint.load_training_state(ckpt) if ckpt else None
    if ckpt is not None and ckpt["trainer"]["epoch"] >= training_cfg["epochs"]:
        comm.barrier()
        return ckpt["trainer"]["history"]           # the run had finished: nothing is built, nothing is written
    dev = torch.device("cpu") if cpu else torch.device("cuda", comm.local_rank)
    if not cpu:
        torch.cuda.set_device(dev)
    elif model_cfg.get("name") != "ConvTasNet":
        raise NotImplementedError("--use_cpu: the CPU backend serves the ConvTasNet step (cfg 1 of BASELINE.json) only")

    model_cfg.update({"model_path": training_cfg.get("pretrained", None)})
    pre = model_cfg["model_path"]
    if ckpt is not None and pre is not None and not str(pre).startswith("https") and not os.path.exists(pre):
        # the checkpoint holds the student AND the teacher: a pretrained file that has moved since the first launch is not needed
        print(f"Resuming: pretrained file {pre} is gone; the teacher comes from the checkpoint")
        model_cfg["model_path"] = None
    model, fmodel = create_pretrained_model(model_cfg)
    model.to(dev).train()
    fmodel.to(dev).eval()
    if comm.rank == 0:
        os.makedirs(work_dir, exist_ok=True)
        with open(os.path.join(work_dir, "conf.yml"), "w") as out:
            for blk in (model_cfg, dataset_cfg, training_cfg):
                yaml.safe_dump(blk, out)

    opt = training_cfg.get("optim", {})
    # make_optimizer(**training_cfg["optim"]) of the reference (asteroid_librimix_trainer.py:94): adam, adamw and sgd have a fused clip +
    # update kernel (fqss_adam_clip / fqss_optim_clip); any other name is refused rather than silently replaced
    opt_name = str(opt.get("optimizer", "adam")).lower()
    if opt_name not in ("adam", "adamw", "sgd"):
        raise NotImplementedError(f"asteroid env: optim.optimizer {opt.get('optimizer')!r}: one of adam, adamw, sgd has a fused kernel")
    optim = dict(optimizer=opt_name, weight_decay=float(opt.get("weight_decay", 0) or 0), momentum=float(opt.get("momentum", 0) or 0),
                 nesterov=bool(opt.get("nesterov", False)))
    betas = tuple(opt.get("betas", (0.9, 0.999)))
    data = _Data(dataset_cfg, training_cfg, comm, dev, n_src=model_cfg.get("n_src", 2))
    # the loader's next mixture is on the device a step early: the frozen teacher runs on it beside the current step (KDTrainStep
    # teacher_ahead: the path bench.py measures; HIP backend only)
    ahead = (not cpu) and training_cfg.get("kd_lambda", 0) > 0 and bool(training_cfg.get("teacher_ahead", True))
    system = System(model, fmodel, training_cfg.get("kd_lambda", 0), lr=opt.get("lr", 1e-3), clip=5.0, comm=comm, betas=betas,
                    teacher_ahead=ahead, accumulate=training_cfg.get("accumulate_grad_batches", 1), **optim)
    global LAST_SYSTEM
    LAST_SYSTEM = system                # tools / tests: the stepper of the run that just finished (its graphs, its model)
    best, history, since_best, first_epoch = float("inf"), [], 0, 0
    # schedulers of train_setup (asteroid_librimix_trainer.py:96-102): StepLR for `step_lr` (DPTNet config), ReduceLROnPlateau
    # (factor 0.5) for `half_lr`; both act once per epoch on the stepper's learning rate
    step_lr, half_lr = training_cfg.get("step_lr"), training_cfg.get("half_lr", False)
    base_lr, plateau_best, plateau_bad = opt.get("lr", 1e-3), float("inf"), 0
    if ckpt is not None:
        # student, arena, quantizer state (the stored per-quantizer observer flags, not the YAML's `observer`), learning rate, teacher
        # and random streams from the file; then this loop's own bookkeeping.  StepLR needs nothing stored beyond the epoch number.
        ts = checkpoint.restore(ckpt, system.stepper, fmodel)
        best, since_best, first_epoch, history = ts["best"], ts["since_best"], ts["epoch"], list(ts["history"])
        plateau_best, plateau_bad = ts["plateau_best"], ts["plateau_bad"]
        if comm.rank == 0:
            print(f"Resuming after epoch {first_epoch}: best val_loss {best}, lr {system.stepper.lr}", flush=True)
    for epoch in range(first_epoch, training_cfg["epochs"]):
        if training_cfg.get("early_stop", False) and since_best >= 30:      # (a resumed run that had stopped early stays stopped)
            break
        import time
        t_epoch, n_steps = time.perf_counter(), 0
        for i, (x, tgt, x_next) in enumerate(data.train(epoch)):
            system.training_step((x, tgt), i, x_next=x_next)
            n_steps += 1
        # accumulate_grad_batches (pl.Trainer): an epoch that ends inside a window updates on what the window holds, before the
        # validation and the checkpoint
        system.stepper.flush()
        if not cpu:
            torch.cuda.synchronize()
        t_epoch = time.perf_counter() - t_epoch
        val = torch.stack([system.validation_step(b, i) for i, b in enumerate(data.val(epoch))]).mean()
        comm.all_reduce_sum(val)
        val = val.item() / comm.world
        history.append({"epoch": epoch, "loss": system.logged["loss"].item(), "val_loss": val, "lr": system.stepper.lr,
                        "train_ms_per_step": 1e3 * t_epoch / max(1, n_steps), "loader_wait_s": data.loader_wait_s,
                        "launch": "hipGraph replay" if system.stepper._graphs is not None else "eager"})
        if half_lr:
            if val < plateau_best - 1e-4 * abs(plateau_best):     # torch ReduceLROnPlateau defaults: rel threshold 1e-4
                plateau_best, plateau_bad = val, 0
            else:
                plateau_bad += 1
                if plateau_bad > training_cfg.get("patience", 5):
                    system.stepper.lr, plateau_bad = system.stepper.lr * 0.5, 0
        elif step_lr is not None:
            system.stepper.lr = base_lr * step_lr.get("gamma", 0.98) ** ((epoch + 1) // step_lr.get("step_size", 2))
        if comm.rank == 0:
            print(json.dumps(history[-1]), flush=True)
            sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
            torch.save(sd, os.path.join(work_dir, "latest_model.pth"))
            if val < best:
                torch.save(sd, os.path.join(work_dir, "best_model.pth"))
        # EarlyStopping(monitor="val_loss", mode="min", patience=30) of train_setup (:117-118); every rank sees the same reduced `val`
        since_best = 0 if val < best else since_best + 1
        best = min(best, val)
        checkpoint.save_training_state(os.path.join(work_dir, checkpoint.NAME), system.stepper,
                                       dict(epoch=epoch + 1, best=best, since_best=since_best, plateau_best=plateau_best,
                                            plateau_bad=plateau_bad, history=history), fmodel)
        if training_cfg.get("early_stop", False) and since_best >= 30:
            if comm.rank == 0:
                print(f"Early stopping: val_loss has not improved for {since_best} epochs")
            break
    comm.barrier()
    return history
