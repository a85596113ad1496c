"""Host reductions (shm transport, ec_cpu::reduce) against the exact model
of tests/numerics_cases.py: ties, subnormals, overflow, NaN / inf / signed
zero, the AVG scale at 3 and 7 ranks and the integer extremes, every
message compared bit for bit with no tolerance. The rule tested is the
"Reduction numerics" section of docs/USER_GUIDE.md."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numerics_cases as nc  # noqa: E402
from ucc_amd.testing import LocalJob  # noqa: E402

_JOBS = {}


def _job(n):
    if n not in _JOBS:
        _JOBS[n] = LocalJob(n)
    return _JOBS[n]


def _allreduce_host(case):
    job = _job(case.n)
    srcs = [np.frombuffer(x, dtype=np.uint8).copy() for x in case.x]
    dsts = [np.full(case.nbytes, 0xA5, dtype=np.uint8) for _ in srcs]
    reqs = job.coll("allreduce", [
        dict(src=srcs[r].ctypes.data, dst=dsts[r].ctypes.data,
             count=case.count, dt=case.dt, op=case.op)
        for r in range(case.n)
    ])
    job.run(reqs)
    return dsts


def test_case_table():
    """every family is there, at 3 ranks and (AVG) at 7"""
    fam3 = {c.family for c in nc.cases(3)}
    assert fam3 == {"ties", "subnormal", "overflow", "specials", "avgscale",
                    "intext"}
    assert {c.family for c in nc.cases(7)} == \
        {"ties", "subnormal", "specials", "avgscale"}
    assert all(c.count % nc.vec_of(c.dt) != 0
               for n in (3, 7) for c in nc.cases(n) if nc.vec_of(c.dt) > 1)
    assert min(c.nbytes for n in (3, 7) for c in nc.cases(n)) >= nc.MIN_BYTES


@pytest.mark.parametrize("case", nc.cases(3) + nc.cases(7),
                         ids=lambda c: c.id)
def test_host_reduce(case):
    for d in _allreduce_host(case):
        assert case.mismatch(d.tobytes()) is None
