"""Worker for tests/test_reduce_numerics_gpu.py: every 3-rank message of
tests/numerics_cases.py as a cross-process allreduce on cuda:0, compared
bit for bit with the exact model. Run under
  python -m torch.distributed.run --nnodes=1 --nproc-per-node=3 \
      --master-addr 127.0.0.1 tests/numerics_worker.py fused|gated

fused: default thresholds, these 17..176-byte messages take the fused
small-message kernel. gated: the test lowers UCC_TL_CDNA4_FUSED_MAX below
the smallest message; every case then runs once as a one-shot request
(stage / k_staged_reduce / gather kernels) and once as a persistent one
(zero-copy, one k_zc_allreduce launch).
"""

import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ucc_amd import core, dtypes  # noqa: E402
import numerics_cases as nc  # noqa: E402
from dispatch_worker import oob, wait  # noqa: E402


def main():
    mode = sys.argv[1]
    rank = int(os.environ["RANK"])
    world = int(os.environ["WORLD_SIZE"])
    assert world == 3
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    c = core()
    lib = c.Lib()
    ctx = c.Context(lib)
    team = c.team_create_post(ctx, py_allgather=oob(dist.group.WORLD, world),
                              rank=rank, n_ranks=world)
    while True:
        st = c.team_create_test(team)
        if st == c.OK:
            break
        if st < 0:
            raise RuntimeError(f"team create failed: {st}")

    bad = []
    cases = nc.cases(world)
    flag_sets = [0] if mode == "fused" else [0, c.FLAG_PERSISTENT]
    for case in cases:
        for flags in flag_sets:
            src = torch.frombuffer(bytearray(case.x[rank]),
                                   dtype=torch.uint8).cuda()
            dst = torch.full_like(src, 0xA5)
            # the fill runs on torch's stream, the collective on the
            # library's: finish the fill before the kernels may write dst
            torch.cuda.synchronize()
            req = c.coll_init(team, "allreduce", src=src.data_ptr(),
                              dst=dst.data_ptr(), count=case.count,
                              dt=case.dt, op=case.op,
                              mem_type=dtypes.MEM_CUDA, flags=flags)
            wait(req, ctx)
            torch.cuda.synchronize()
            m = case.mismatch(dst.cpu().numpy().tobytes())
            if m:
                bad.append(f"flags={flags} {m}")
            del req

    dist.barrier()
    for b in bad:
        print(f"NUM_BAD rank={rank} {b}", flush=True)
    print(f"NUM_DONE rank={rank} mode={mode} cases={len(cases)} "
          f"bad={len(bad)}", flush=True)
    dist.destroy_process_group()
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
