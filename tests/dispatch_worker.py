"""Worker for tests/test_ec_dispatch_gpu.py: every supported (dtype, op)
cell of tests/dispatch_cases.py as a cross-process 2-rank allreduce on
cuda:0, compared exactly with the host model; every unsupported cell must
be refused at coll_init. Run under
  python -m torch.distributed.run --nnodes=1 --nproc-per-node=2 \
      --master-addr 127.0.0.1 tests/dispatch_worker.py fused|gated

fused: default thresholds, these 51..102-byte messages take the fused
small-message kernel. gated: the test lowers UCC_TL_CDNA4_FUSED_MAX below
the smallest message; every cell then runs once as a one-shot request
(stage / reduce / gather kernels) and once as a persistent one (zero-copy,
one k_zc_allreduce launch).
"""

import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ucc_amd import core, dtypes  # noqa: E402
import dispatch_cases as dc  # noqa: E402


def oob(group, world):
    def allgather(data: bytes):
        n = len(data)
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8).clone()
        outs = [torch.empty(n, dtype=torch.uint8) for _ in range(world)]
        dist.all_gather(outs, t, group=group)
        return [o.numpy().tobytes() for o in outs]

    return allgather


def wait(req, ctx):
    req.post()
    it = 0
    while req.test() == core().INPROGRESS:
        ctx.progress()
        it += 1
        if it > 200_000_000:
            raise TimeoutError("collective stuck")


def main():
    mode = sys.argv[1]
    rank = int(os.environ["RANK"])
    world = int(os.environ["WORLD_SIZE"])
    assert world == 2
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
    flag_sets = [0] if mode == "fused" else [0, c.FLAG_PERSISTENT]
    for dt, op in dc.CELLS:
        x = dc.inputs(dt, op)
        for flags in flag_sets:
            src = dc.to_device(dt, x[rank])
            dst = torch.zeros_like(src)
            req = c.coll_init(team, "allreduce", src=src.data_ptr(),
                              dst=dst.data_ptr(), count=dc.count_for(dt),
                              dt=dt, op=op, mem_type=dtypes.MEM_CUDA,
                              flags=flags)
            wait(req, ctx)
            torch.cuda.synchronize()
            m = dc.mismatch(dt, op, x, dst)
            if m:
                bad.append(f"flags={flags} {m}")
            del req

    refused = 0
    buf = torch.zeros(256, dtype=torch.uint8, device="cuda")
    out = torch.zeros(256, dtype=torch.uint8, device="cuda")
    for dt, op in dc.UNSUPPORTED:
        try:
            c.coll_init(team, "allreduce", src=buf.data_ptr(),
                        dst=out.data_ptr(), count=dc.count_for(dt), dt=dt,
                        op=op, mem_type=dtypes.MEM_CUDA)
            bad.append(f"{dc.cell_id((dt, op))}: accepted")
        except RuntimeError as e:
            if "Not supported" in str(e):
                refused += 1
            else:
                bad.append(f"{dc.cell_id((dt, op))}: {e}")

    dist.barrier()
    for b in bad:
        print(f"DISPATCH_BAD rank={rank} {b}", flush=True)
    print(f"DISPATCH_DONE rank={rank} mode={mode} cells={len(dc.CELLS)} "
          f"refused={refused} bad={len(bad)}", flush=True)
    dist.destroy_process_group()
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
