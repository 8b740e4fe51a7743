"""One data-parallel rank of tests/test_gpu_resume.py::test_two_ranks_resume_with_their_own_observer_ranges (a fresh process, both ranks
on GPU 0, gloo transport, like tests/ddp_worker.py): the tiny ConvTasNet inside the observer phase on per-rank shards, the training
state written through fqss_amd.checkpoint (every rank's ranges and n_iter gathered, rank 0 writes), then NEW model objects and a new
KDTrainStep resumed from the file at the same world size, the rest of the observer phase, the one-time range synchronisation, two steps.

    python -m tests.resume_ddp_worker <rank> <world> <port> <out.pt> <checkpoint.pth>
"""
import os
import sys

import numpy as np


def main():
    rank, world, port, out, ckpt = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                      FQSS_DIST_BACKEND="gloo")
    import torch
    from fqss_amd import checkpoint, ops
    from fqss_amd.parallel import Comm
    from fqss_amd.runtime import KDTrainStep
    from tests.ddp_worker import shard
    from tests.test_gpu_model import T, _tiny_pair
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "tiny_step.npz"))
    comm = Comm.from_env("cuda")
    assert comm.world == world and comm.rank == rank
    xr, tr = shard(T(g["x"]).cuda(), T(g["tgt"]).cuda(), rank, world)
    kw = dict(kd_lambda=0.1, lr=1e-3, clip=5.0, comm=comm, buckets=2)
    ranges = lambda model: {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if "activation_fake_quantize" in k}
    n_iter = lambda step: sorted({m.n_iter for _, m in step._quantizers()[0]})
    res = {}
    with ops.poison_carriers(True):
        model, fmodel = _tiny_pair(g)
        step = KDTrainStep(model, fmodel, **kw)
        step(xr, tr)                                  # call 1 with a backward (weight observers, first Adam step)
        with torch.no_grad():
            for _ in range(9):
                model(xr)
        assert not step._ranges_synced and not step.can_capture()
        res["saved"], res["n_iter_saved"] = ranges(model), n_iter(step)[0]
        checkpoint.save_training_state(ckpt, step, dict(epoch=0), fmodel)
        del step, model, fmodel
        # a NEW launch: fresh objects, everything from the file
        model, fmodel = _tiny_pair(g)
        step = KDTrainStep(model, fmodel, **kw)
        assert checkpoint.restore(checkpoint.load_training_state(ckpt), step, fmodel) == dict(epoch=0)
        res["loaded"], res["n_iter_loaded"], res["synced_loaded"] = ranges(model), n_iter(step)[0], step._ranges_synced
        with torch.no_grad():
            for _ in range(50 - res["n_iter_loaded"]):
                model(xr)
        assert step.can_capture() and not step._ranges_synced
        step._maybe_sync_ranges()
        res["synced_end"], res["end"] = step._ranges_synced, ranges(model)
        res["losses"] = [step(xr, tr)["loss"].item() for _ in range(2)]      # quantizing steps on the common grid
    torch.cuda.synchronize()
    torch.save(res, out)
    comm.barrier()
    comm.close()


if __name__ == "__main__":
    main()
