"""`main()` of the htdemucs env (reference: train_env/htdemucs_musdbhq/train.py:163-262 `get_solver` / `main`, solver.py:38-429
`Solver`), MI355X edition, without the hydra / dora / demucs dependencies.

Plugin surface kept: `main()` takes no arguments and reads `key=value` / `+key=value` overrides from `sys.argv[1:]` the way the
reference's hydra entry point does (train.py:44-46 passes `+device=<device>`); the configuration is the reference's YAML layout
(`model_cfg{,.quantization}`, `dset`, `epochs`, `batch_size`, `optim{lr, beta2, loss, clip_grad, weight_decay}`, `weights`,
`kd_lambda`, `seed`, `test.metric`).  `+yml_path=<file>` selects the YAML (default: configs/htdemucs_synthetic.yaml); the
reference always reads configs/htdemucs.yaml through hydra.  Step semantics kept (solver.py:314-429):
  * train: mix = sum of the stems; estimate = student(mix); teacher under no_grad; loss = source-weighted
    (1 - kd_lambda) L1(est, src) + kd_lambda w L1(est, teacher), w = exp((sdr_teacher - sdr_student) / 10) per (sample, source);
    optional clip_grad; Adam(lr, betas (momentum, beta2)); global batch divided over the ranks (train.py:200-201), gradients
    averaged over ranks;
  * valid: eval mode on the validation stems, `reco` = source-weighted L1; the best state by `test.metric: loss` is written to
    `<work_dir>/best.th` as {"state", "kwargs", "history"} (the keys load_model.py:38-45, 76-102 read back);
  * every epoch ends with `<work_dir>/checkpoint.pth`, the full training state (the place of the solver's checkpoint.th); `resume=<path>`
    or `resume=auto` continues from one (fqss_amd/checkpoint.py).
Data: `dset.name: synthetic` (seeded Gaussian stems), or folders of WAV stems (`dset.wav` / `dset.musdb` + `use_musdb`, wav_dataset.py):
a prefetching reader a batch ahead of the step, int16 samples to the device, demucs' augmentations (shift / flip / scale / remix, restated)
and the mixture in one fused kernel; validation is un-augmented windows of the training length.  demucs' repitch, EMA copies,
`apply_model` split inference and the SDR evaluation are the reference's CPU / third-party data side."""
import json
import os
import sys

import torch
import yaml

from ... import checkpoint
from ...parallel import Comm, local_device
from ...quantization.qat.models.load_model import quantize_model
from ...quantization.qat.models.htdemucsq import HTDemucsQ
from ...runtime import KDTrainStep
from ...utils import set_seed
from ... import kernels as K
from ...loader import Prefetcher, epoch_batches
from . import wav_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def _set_path(conf, dotted, value):
    cur = conf
    keys = dotted.split(".")
    for k in keys[:-1]:
        cur = cur.setdefault(k, {})
    cur[keys[-1]] = value


def load_config(argv):
    """hydra-style overrides: `a.b=1`, `+a.b=1`; values are parsed as YAML scalars"""
    over = {}
    for tok in argv:
        if "=" not in tok:
            raise ValueError(f"override {tok!r}: expected key=value")
        k, v = tok.lstrip("+").split("=", 1)
        over[k] = yaml.safe_load(v)
    path = over.pop("yml_path", None) or os.path.join(ROOT, "configs", "htdemucs_synthetic.yaml")
    conf = yaml.safe_load(open(path))
    for k, v in over.items():
        _set_path(conf, k, v)
    return conf


def synth_stems(B, S, C, T, seed, device):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, S, C, T, generator=g) * 0.1).to(device)


def group_decays(model):
    """{parameter name: weight decay} of the modules that form an optimizer group of their own in the reference (make_optim_group,
    htdemucsq.py:525-529: the cross-transformer, with its `weight_decay` attribute -- t_weight_decay).  A group learning rate is not
    built: it is None in every configuration."""
    from ...quantization.qat.models.htdemucsq import CrossTransformerEncoder
    out = {}
    for name, module in model.named_modules():
        if isinstance(module, CrossTransformerEncoder):
            if module.lr is not None:
                raise NotImplementedError(f"htdemucs env: {name} asks for a learning rate of its own (t_lr = {module.lr}); not built")
            for n, p in module.named_parameters():
                if p.requires_grad:
                    out[f"{name}.{n}" if name else n] = float(module.weight_decay)
    return out


class Solver:
    def __init__(self, conf, model, fmodel, comm, device):
        self.conf, self.model, self.fmodel, self.comm, self.device = conf, model, fmodel, comm, device
        opt = conf["optim"]
        if opt.get("loss", "l1") != "l1":
            raise NotImplementedError("htdemucs env: optim.loss: the L1 loss is the one that is built")
        # get_optimizer (train.py:88-119): Adam or AdamW over the model, the modules with a make_optim_group() -- the cross-transformer --
        # in a group of their own, with their own weight decay whatever optim.weight_decay says
        kind = str(opt.get("optim", "adam")).lower()
        if kind not in ("adam", "adamw"):
            raise ValueError(f"htdemucs env: optim.optim {opt.get('optim')!r}: adam or adamw")
        self.weights = torch.tensor(conf.get("weights", [1.0] * model.n_srcs), device=device, dtype=torch.float32)
        ema = conf.get("ema") or {}
        self.step = KDTrainStep(model, fmodel, kd_lambda=float(conf.get("kd_lambda", 0.1)), lr=float(opt["lr"]),
                                clip=float(opt.get("clip_grad") or 0.0), comm=comm, loss="l1_sdr", source_weights=self.weights,
                                betas=(float(opt.get("momentum", 0.9)), float(opt.get("beta2", 0.999))),
                                accumulate=opt.get("accumulate_grad_batches", 1),    # ours (demucs has none): micro-batches per update
                                optimizer=kind, weight_decay=float(opt.get("weight_decay", 0) or 0), param_decay=group_decays(model),
                                ema_decays=tuple(ema.get("batch") or ()), ema_epoch_decays=tuple(ema.get("epoch") or ()))
        self.history = []
        self.best_state, self.best_loss = None, float("inf")
        self.ckpt_file = os.path.join(conf["work_dir"], checkpoint.NAME)
        self.sets = None
        if wav_dataset.configured(conf["dset"]):
            # refusals first (repitch, a per-GPU batch the remix groups do not divide): nothing is read before them
            wav_dataset.check_augment_cfg(conf.get("augment"), conf["batch_size"] // comm.world)
            train_set, valid_set = wav_dataset.build_datasets(conf, device)
            if len(train_set.sources) != model.n_srcs:
                raise ValueError(f"dset.sources names {len(train_set.sources)} stems, the model separates {model.n_srcs}")
            self.sets = {True: train_set, False: valid_set}

    def restore(self, ckpt):
        """student, arena, quantizer state, learning rate, teacher and random streams from a training-state checkpoint; then the
        solver's own fields.  The next epoch is len(history)."""
        ts = checkpoint.restore(ckpt, self.step, self.fmodel)
        self.history, self.best_loss, self.best_state = list(ts["history"]), ts["best_loss"], ts["best_state"]
        if self.comm.rank == 0:
            print(f"Resuming after epoch {len(self.history)}: best {self.best_loss}", flush=True)

    def _batch(self, epoch, idx, train):
        d = self.conf["dset"]
        B = self.conf["batch_size"] // self.comm.world if train else 1
        T = int(round(d["segment"] * d["samplerate"]))
        seed = self.conf.get("seed", 42) * 1000003 + (epoch * 4096 + idx) * self.comm.world + self.comm.rank + (0 if train else 1 << 30)
        return synth_stems(B, self.model.n_srcs, d["channels"], T, seed, self.device)

    def _wav_batches(self, epoch, train):
        """this rank's batches of the epoch: torch's sampler order (loader.epoch_batches), the single-process permutation drawn from a
        generator of (seed, epoch) instead of the global RNG, so which examples land in a batch depends on the epoch number alone; a
        training batch carries the seed of its position, so the reader draws the same augmentation for it in any run that gets there"""
        conf, comm, ds = self.conf, self.comm, self.sets[train]
        B = conf["batch_size"] // comm.world if train else 1
        seed = conf.get("seed", 42)
        order = torch.Generator().manual_seed(int(seed) * 1000003 + int(epoch))
        batches = epoch_batches(len(ds), B, shuffle=train, drop_last=True, rank=comm.rank, world=comm.world, seed=seed, epoch=epoch,
                                generator=order)
        caps = [conf.get("max_batches")] + ([] if train else [conf["dset"].get("valid_steps")])
        for cap in caps:
            if cap is not None:
                batches = batches[:int(cap)]
        if not batches:
            raise ValueError(f"htdemucs env: the {'training' if train else 'validation'} set of {len(ds)} examples gives no batch of {B}")
        if train:
            batches = [wav_dataset.SeededBatch(b, wav_dataset.batch_seed(seed, epoch, i, comm.rank, comm.world)) for i, b in enumerate(batches)]
        return batches

    def _synthetic_batches(self, epoch, n, train):
        for idx in range(n):
            sources = self._batch(epoch, idx, train)
            yield sources.sum(dim=1), sources

    def _run_one_epoch(self, epoch, train=True):
        pf = None
        if self.sets is not None:
            batches = self._wav_batches(epoch, train)
            n = len(batches)
            it = pf = Prefetcher(self.sets[train], batches, self.device, depth=int(self.conf.get("prefetch_depth", 2)))
        else:
            d = self.conf["dset"]
            n = d["steps_per_epoch"] if train else d["valid_steps"]
            it = self._synthetic_batches(epoch, n, train)
        tot = torch.zeros(1, device=self.device, dtype=torch.float64)
        self.model.train(train)
        for mix, sources in it:
            if train:
                self.step.maybe_capture(mix, sources)
                tot += self.step(mix, sources)["loss"].double()
            else:
                with torch.no_grad():
                    est = self.model(mix)
                    loss, task, _, _, _ = K.hd_kd_loss(est, est, sources, self.weights, 0.0, want_grad=False)    # kd_lambda 0: the L1 task loss
                tot += loss.double()
        if train:
            self.step.flush()       # optim.accumulate_grad_batches: a window the epoch cut short updates on what it holds
            self.step.ema_epoch_update()    # ema.epoch: once per epoch, after training (solver.py:438-440)
        self.comm.all_reduce_sum(tot)
        out = {"loss": tot.item() / (n * self.comm.world), "reco": tot.item() / (n * self.comm.world)}
        if train:
            out["launch"] = "hipGraph replay" if self.step._graphs is not None else "eager"
        if pf is not None:
            out["loader_wait_s"] = pf.wait_s      # host time this loop spent blocked on the reader (a loader that keeps up: ~0)
        return out

    def train(self):
        for epoch in range(len(self.history), self.conf["epochs"]):
            m = {"train": self._run_one_epoch(epoch), "valid": self._run_one_epoch(epoch, train=False)}
            self.model.train()
            key = self.conf.get("test", {}).get("metric", "loss")
            if key != "loss":
                raise NotImplementedError("htdemucs env: best-model selection by nsdr needs demucs' evaluation (third party)")
            # the EMA copies are validated with the model's own pass; the best of them all by `loss` is the epoch's candidate for
            # best_state, under the name the reference records (solver.py:220-236)
            # (a run without copies keeps the history it always wrote: `valid` is the model's own pass)
            bcopy = None
            if self.step.ema_kinds:
                main = m["valid"]
                m["valid"] = {"main": main}
                bvalid, bname = main, "main"
                for k, kind in enumerate(self.step.ema_kinds):
                    name = f"ema_{kind}_{self.step.ema_kinds[:k].count(kind)}"
                    with self.step.ema_swap(k):
                        v = self._run_one_epoch(epoch, train=False)
                    m["valid"][name] = v
                    if v["loss"] < bvalid["loss"]:
                        bvalid, bname, bcopy = v, name, k
                m["valid"].update(bvalid)
                m["valid"]["bname"] = bname
            self.model.train()
            if m["valid"]["loss"] <= self.best_loss:
                self.best_loss = m["valid"]["loss"]
                state = self.model.state_dict() if bcopy is None else self.step.ema_state(bcopy)
                self.best_state = {k: v.detach().cpu().clone() for k, v in state.items()}
            m["valid"]["best"] = self.best_loss
            self.history.append(m)
            if self.comm.rank == 0:
                print(f"epoch {epoch + 1}: train loss {m['train']['loss']:.5f}  valid loss {m['valid']['loss']:.5f}  best {self.best_loss:.5f}",
                      flush=True)
                os.makedirs(self.conf["work_dir"], exist_ok=True)
                torch.save({"state": self.best_state, "kwargs": self.model._init_kwargs, "history": self.history},
                           os.path.join(self.conf["work_dir"], "best.th"))
                with open(os.path.join(self.conf["work_dir"], "history.json"), "w") as f:
                    json.dump(self.history, f)
            checkpoint.save_training_state(self.ckpt_file, self.step, dict(epoch=epoch + 1, history=self.history, best_loss=self.best_loss,
                                                                           best_state=self.best_state), self.fmodel)
        return self.history


def get_solver(conf, ckpt=None):
    """ckpt: a loaded training-state checkpoint to continue from (main() resolves the `resume` key)"""
    import copy
    device = conf.get("device", "cuda")
    if device != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("the htdemucs env of this build trains on ROCm devices only (no CPU fallback; oracle/ is the CPU checker)")
    comm = Comm.from_env("cuda")
    torch.cuda.set_device(local_device(comm.local_rank))
    dev = torch.device("cuda", torch.cuda.current_device())
    set_seed(conf.get("seed", 42))
    mc = conf["model_cfg"]
    kwargs = dict(sources=list(conf["dset"]["sources"]), audio_channels=conf["dset"]["channels"], samplerate=conf["dset"]["samplerate"],
                  segment=conf["dset"]["segment"])
    kwargs.update(conf.get("htdemucs") or {})
    model = HTDemucsQ(**kwargs)
    model._init_kwargs = kwargs
    if mc.get("model_path"):
        sd = torch.load(mc["model_path"], map_location="cpu", weights_only=False)   # trusted local package ({"state", "kwargs"})
        model.load_state_dict(sd.get("state", sd), strict=True)
    fmodel = copy.deepcopy(model).to(dev).eval() if float(conf.get("kd_lambda", 0.1)) > 0 else None
    if fmodel is None:
        raise NotImplementedError("htdemucs env: kd_lambda = 0 (no teacher) is not built; the shipped value is 0.1")
    model = quantize_model(model, mc["quantization"]).to(dev).train()
    model._init_kwargs = kwargs
    assert conf["batch_size"] % comm.world == 0
    solver = Solver(conf, model, fmodel, comm, dev)
    if ckpt is not None:
        solver.restore(ckpt)
    return solver


def main():
    conf = load_config(sys.argv[1:])
    # `resume=<path> | auto`: a run that had finished returns its stored history -- nothing is built, nothing is written
    ckpt = checkpoint.resume_path(conf.get("resume"), conf["work_dir"])
    ckpt = checkpoint.load_training_state(ckpt) if ckpt else None
    if ckpt is not None and ckpt["trainer"]["epoch"] >= conf["epochs"]:
        return ckpt["trainer"]["history"]
    solver = get_solver(conf, ckpt)
    hist = solver.train()
    solver.comm.close()
    return hist
