"""The exchange schedule of gradient accumulation at world 1 (tests/test_gpu_accum.py), in a fresh process: a one-rank RCCL
communicator with the world > 1 schedule forced on (FQSS_FORCE_DIST=1, FQSS_FORCE_BUCKETS=1), two gradient buckets, windows of two
micro-batches -- the first window eager, the second replayed from the hipGraphs.  Every call of the communicator's all-reduce is
counted per micro-batch; the same two windows run beside it on a step without a communicator (all-reduce(SUM) over one rank is the
identity, and FQSS_DETERMINISTIC=1 takes the atomics' order out of both).

    python -m tests.accum_worker <port> <out.pt>
"""
import os
import sys


def main():
    port, out = sys.argv[1], sys.argv[2]
    os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port, FQSS_DIST_BACKEND="nccl",
                      FQSS_FORCE_DIST="1", FQSS_FORCE_BUCKETS="1", FQSS_DETERMINISTIC="1")
    import torch
    from fqss_amd.parallel import Comm
    from tests.test_accum_cpu import ab, make_step, settle, snapshot
    from tests.test_gpu_model import TINY
    comm = Comm.from_env("cuda")
    assert comm.backend == "nccl" and comm.active and comm.world == 1
    calls = []
    inner = comm.all_reduce_sum
    comm.all_reduce_sum = lambda t: (calls.append(t.numel()), inner(t))[1]
    # one state past the observer phase, loaded into both steps (by parameter name: the bucketed arenas are in segment order)
    sd = settle(make_step("cuda", TINY), "cuda").state_dict()
    alone = make_step("cuda", TINY, buckets=2, accumulate=2)
    ranked = make_step("cuda", TINY, buckets=2, accumulate=2, comm=comm)
    assert ranked._exchange() and not alone._exchange()
    assert ranked.segments is not None and len(ranked.segments) == 2 and ranked.segments == alone.segments
    res = {"bucket_elems": [hi - lo for lo, hi in ranked.segments], "per_micro_batch": [], "losses": []}
    for step in (alone, ranked):
        step.load_state_dict(sd)
    A, B = ab("cuda")
    for window in range(2):
        for step in (alone, ranked):
            if window == 1:
                step.capture(A[0], A[1], warmup=0)
                assert len(step._graphs[0]) == 2 and getattr(step, "_graph_all", None) is None
            for x, tgt in (A, B):
                del calls[:]
                r = step(x, tgt)
                torch.cuda.synchronize()
                if step is ranked:
                    res["per_micro_batch"].append(list(calls))
                    res["losses"].append(r["loss"].item())
            assert step.pending == 0
    res["alone"], res["ranked"] = ({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in snapshot(s).items()} for s in (alone, ranked))
    torch.save(res, out)
    comm.barrier()
    comm.close()


if __name__ == "__main__":
    main()
