"""The fused one-kernel allgather / reduce_scatter / alltoall / bcast /
reduce of tl/cdna4 (UCC_TL_CDNA4_FUSED_COLLS=1): tests/fused_colls_worker.py
runs seeded exact-integer cases and compares every destination bit for bit.
Four torchrun launches in total (ranks share cuda:0), shared by all tests
of this file; the worker's docstring lists the modes.

Selection is read from the UCC_COLL_TRACE lines: every rank writes down for
every request of the five types whether it must trace cdna4/fused, and the
multiset of trace lines must match."""

import collections
import glob
import os
import re
import sys

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_zc_fused_gpu import _torchrun  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, "tests", "fused_colls_worker.py")

HOST_KERNEL = "host-sequenced kernel (k_fused_coll)"
GRAPH_KERNEL = "graph kernel (k_fused_coll_graph)"
FIVE = ("allgather", "reduce_scatter", "alltoall", "bcast", "reduce")

ENV = {
    "UCC_TL_CDNA4_FUSED_COLLS": "1",
    "UCC_TL_CDNA4_FUSED_COLLS_MAX": "524288",
    "UCC_COLL_TRACE": "1",
    "UCC_LOG_LEVEL": "debug",
}
ENV_OFF = {"UCC_TL_CDNA4_FUSED_COLLS": "0", "UCC_COLL_TRACE": "1",
           "UCC_LOG_LEVEL": "debug"}

TRACE = re.compile(r"coll (\w+) mem \w+ size (\d+) -> (\w+)/(\w+) ")
REQ = re.compile(r"^FC_REQ (\w+) (\d+) ([FO])$", re.M)
POSTS = re.compile(r"^FC_POSTS (\d+)$", re.M)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = {}
    for mode, nproc, env in (("all", 2, ENV), ("three", 3, ENV),
                             ("trig", 2, ENV), ("off", 2, ENV_OFF)):
        d = tmp_path_factory.mktemp(mode)
        proc = _torchrun([WORKER, str(d), mode], timeout=240, env_extra=env,
                         nproc=nproc)
        proc.notes = "".join(open(f).read() for f in
                             sorted(glob.glob(os.path.join(str(d), "*.txt"))))
        sys.stdout.write(f"--- {mode}: rc={proc.returncode}\n")
        sys.stdout.write(proc.stdout[-1500:])
        sys.stderr.write("\n".join(
            ln for ln in proc.stderr.splitlines()
            if " DEBUG " not in ln and " INFO " not in ln)[-3000:])
        out[mode] = proc
    return out


def _traced(proc):
    """(coll, msgsize, traced cdna4/fused) of every trace line of the five
    types."""
    got = collections.Counter()
    for coll, size, tl, alg in TRACE.findall(proc.stderr):
        if coll in FIVE:
            got[(coll, int(size), (tl, alg) == ("cdna4", "fused"))] += 1
    return got


def _announced(proc):
    return collections.Counter(
        (coll, int(size), f == "F")
        for coll, size, f in REQ.findall(proc.notes))


def _ok(proc, nranks):
    assert proc.returncode == 0
    assert proc.stdout.count("FC_OK") == nranks


def _posts(proc):
    return sum(int(x) for x in POSTS.findall(proc.notes))


@pytest.mark.parametrize("mode,nranks", [("all", 2), ("three", 3)])
def test_results_and_selection(runs, mode, nranks):
    """Every case is bitwise right, bands intact (asserted in the worker);
    every in-bound request of the five types traced cdna4/fused, every
    request over the bound something else."""
    proc = runs[mode]
    _ok(proc, nranks)
    want = _announced(proc)
    assert any(f for (_, _, f) in want) and want == _traced(proc)
    # requests over the bound are among them
    assert any(not f for (_, _, f) in want)
    # one debug line per post, all of the host-sequenced kernel
    assert proc.stderr.count(HOST_KERNEL) == _posts(proc) > 0
    assert GRAPH_KERNEL not in proc.stderr


def test_triggered_and_graph_replay(runs):
    proc = runs["trig"]
    _ok(proc, 2)
    want = _announced(proc)
    assert want == _traced(proc)
    assert all(f for (_, _, f) in want)
    assert sum(want.values()) == 2 * len(FIVE) * 2
    # three eager posts and one capture per request, none host-sequenced
    assert proc.stderr.count(GRAPH_KERNEL) == _posts(proc) == 2 * 10 * 4
    assert HOST_KERNEL not in proc.stderr


def test_knob_unset_keeps_selection(runs):
    proc = runs["off"]
    _ok(proc, 2)
    got = _traced(proc)
    assert got == _announced(proc)
    assert sum(got.values()) == 2 * len(FIVE)
    algs = {coll: alg for coll, _, _, alg in TRACE.findall(proc.stderr)
            if coll in FIVE}
    assert algs == {"allgather": "gated_pipeline",
                    "reduce_scatter": "gated_pipeline",
                    "alltoall": "gated_pipeline",
                    "bcast": "staged_linear", "reduce": "staged_linear"}
    # the score map printed at team creation has no fused entry for them
    assert not re.search(r"^(%s):\w+:\S*@cdna4/fused" % "|".join(FIVE),
                         proc.stderr, re.M)
    assert "allreduce:cuda:" in proc.stderr
    assert HOST_KERNEL not in proc.stderr
