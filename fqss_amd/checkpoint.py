"""Full training-state checkpoints: what an interrupted QAT run needs to go on as if it had never stopped (DESIGN.md "Resuming a run").

`latest_model.pth` / `best_model.pth` / `best.th` hold the student's `state_dict` and serve evaluation and export.  A run stands on
more than that: the Adam moments and clocks of the flat arena, every quantizer's observer counter and flags, whether the ranks have
averaged their ranges yet, the learning rate and the scheduler's bookkeeping, the best validation loss, the history, the frozen
teacher and the host random streams.  The trainers write all of it once per epoch to `<work_dir>/checkpoint.pth` and read it back
when asked to resume (`resume: <path> | auto` in the YAML, `--resume [PATH]` on the command line).

The file is `{"format": "fqss-train-v1", "step", "trainer", "teacher", "rng"}`: tensors and plain Python values only, so
`torch.load(..., weights_only=True)` reads it -- a checkpoint is never a reason to unpickle code.  It is written to a temporary file in
the same directory and moved into place with `os.replace`: a process killed while writing leaves the previous file as it was.
A run on plain Adam without weight decay and without EMA copies writes exactly these keys.  Any other run's `step` entry also says
which optimizer its moments belong to (`optim`: kind, weight_decay, momentum, nesterov, per-parameter decays) and, where the step
keeps EMA copies of the model, carries them (`ema`: kinds, decays, counts, the copies); `KDTrainStep.load_state_dict` refuses a file
of another optimizer kind or another EMA list with a ValueError naming both.
File order needs no entry:`loader.epoch_batches(seed, epoch)` derives it from the epoch number."""
import os
import random

import numpy as np
import torch

FORMAT = "fqss-train-v1"
NAME = "checkpoint.pth"


# ---- host random streams ------------------------------------------------------------------------------------------------------
def rng_state():
    """Python `random`, NumPy's global stream (the LibriMix SNR augmentation draws from it, train_utils.augmentation_2mix), torch's
    CPU generator and the current device's, as tensors / lists"""
    v, words, gauss = random.getstate()
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    out = {"python": [int(v), [int(w) for w in words], gauss],
           "numpy": [str(kind), torch.from_numpy(keys.astype(np.int64)), int(pos), int(has_gauss), float(cached)],
           "torch": torch.get_rng_state().clone(), "device": None}
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        out["device"] = torch.cuda.get_rng_state().clone()
    return out


def set_rng_state(st):
    v, words, gauss = st["python"]
    random.setstate((int(v), tuple(int(w) for w in words), gauss))
    kind, keys, pos, has_gauss, cached = st["numpy"]
    np.random.set_state((str(kind), keys.numpy().astype(np.uint32), int(pos), int(has_gauss), float(cached)))
    torch.set_rng_state(st["torch"].cpu())
    if st.get("device") is not None and torch.cuda.is_available():
        torch.cuda.set_rng_state(st["device"].cpu())


# ---- the file -------------------------------------------------------------------------------------------------------------------
def write_atomic(payload, path):
    """temporary file in the same directory (same file system: the move is atomic), flushed to disk, then os.replace; whatever
    fails on the way, `path` still holds what it held before"""
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    tmp = os.path.join(d, f".{os.path.basename(path)}.{os.getpid()}.tmp")
    try:
        with open(tmp, "wb") as f:
            torch.save(payload, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
        fd = os.open(d, os.O_RDONLY)        # ... and the rename itself: the directory entry reaches the disk too
        try:
            os.fsync(fd)
        finally:
            os.close(fd)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def save_training_state(path, step, trainer_state, teacher):
    """step: the run's KDTrainStep; trainer_state: the trainer's own bookkeeping (epoch, best, scheduler fields, history: plain
    values and tensors); teacher: the frozen float model.  Every rank calls this (step.state_dict() gathers the per-rank observer
    ranges while they differ); rank 0 writes, and a barrier follows the write."""
    comm = step.comm
    sd = step.state_dict()
    if comm is None or comm.rank == 0:
        teacher_sd = {k: v.detach().cpu().clone() for k, v in teacher.state_dict().items()} if teacher is not None else None
        write_atomic({"format": FORMAT, "step": sd, "trainer": trainer_state, "teacher": teacher_sd, "rng": rng_state()}, path)
    if comm is not None:
        comm.barrier()


def load_training_state(path):
    ck = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(ck, dict) or ck.get("format") != FORMAT:
        tag = ck.get("format") if isinstance(ck, dict) else type(ck).__name__
        raise ValueError(f"{path}: not a training-state checkpoint of this build (format {tag!r}, expected {FORMAT!r}); "
                         "latest_model.pth / best_model.pth hold the student's weights only and cannot resume a run")
    return ck


def restore(ck, step, teacher):
    """a loaded checkpoint into a freshly built run: stepper (student, arena, quantizer state), teacher, random streams -> the
    trainer's own state.  The streams come last, so nothing the restore itself draws moves them."""
    step.load_state_dict(ck["step"])
    if teacher is not None and ck.get("teacher") is not None:
        teacher.load_state_dict(ck["teacher"], strict=True)
        step.teacher._planes = None         # (the fused teacher chain splits its weights once: from these, not the fresh ones)
    set_rng_state(ck["rng"])
    return ck["trainer"]


def resume_path(value, work_dir):
    """the trainers' `resume` key -> the file to continue from, or None for a fresh start.  `auto`: `<work_dir>/checkpoint.pth` if it
    exists; anything else is a path that must exist"""
    if value in (None, False, ""):
        return None
    if value is True or str(value).lower() == "auto":
        path = os.path.join(work_dir, NAME)
        return path if os.path.exists(path) else None
    if not os.path.exists(str(value)):
        raise FileNotFoundError(f"resume: {value} does not exist")
    return str(value)
