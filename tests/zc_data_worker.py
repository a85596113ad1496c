"""Worker for tests/test_zc_data_gpu.py: ONE seeded bf16 persistent
allreduce on the zero-copy gated path, run under
  python -m torch.distributed.run --nnodes=1 --nproc-per-node=2 \
      --master-addr 127.0.0.1 tests/zc_data_worker.py OUTDIR SEED COUNT

The test sets UCC_TL_CDNA4_ZC_FUSED=0, so the result comes from the
stage / k_staged_reduce / gather launches. Inputs and the .npy dump are
those of tests/zc_fused_worker.py (Job.inputs, Job.save)."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from zc_fused_worker import Job  # noqa: E402


def main():
    job = Job(sys.argv[1])
    job.allreduce("normals", int(sys.argv[2]), torch.bfloat16,
                  int(sys.argv[3]))
    job.finish("ZCD_OK")


if __name__ == "__main__":
    main()
