"""Device bcast and reduce on the device-gated pipeline
(UCC_TL_CDNA4_GATED_ROOTED=1): tests/gated_rooted_worker.py runs the seeded
cases on cuda:0 — 2 ranks with UCC_TL_CDNA4_ZC_FUSED=1 and =0 (every saved
destination must match bit for bit between the two), 3 ranks, the
stream-triggered posts, and one short run with the knob unset. Five
torchrun launches in total, shared by all tests of this file. What each
case checks is in the worker's docstring."""

import glob
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_zc_fused_gpu import REPO, _torchrun  # noqa: E402

pytestmark = pytest.mark.gpu

WORKER = os.path.join(REPO, "tests", "gated_rooted_worker.py")

ENV = {
    "UCC_TL_CDNA4_GATED_ROOTED": "1",
    "UCC_TL_CDNA4_GATED_BLOCKS": "8",
    "UCC_TL_CDNA4_CHUNK_SIZE": "65536",
    # the allreduce twins of the reduce cases must be gated ones too
    "UCC_TL_CDNA4_FUSED_MAX": "64",
    "UCC_COLL_TRACE": "1",
    "UCC_LOG_LEVEL": "debug",
}

BCAST_ONE = "zero-copy one-kernel (k_zc_bcast) path"
BCAST_THREE = "zero-copy three-kernel (stage/bscatter/wait) path"
REDUCE_ONE = "zero-copy one-kernel (k_zc_allreduce into the root's dst) path"
REDUCE_THREE = ("zero-copy three-kernel (stage/reduce/wait into the root's "
                "dst) path")

TRACE = re.compile(r"coll (bcast|reduce) mem cuda size \d+ -> (\S+)")


def rooted_choices(stderr):
    """{(coll, tl/alg): count} over the selection trace lines."""
    out = {}
    for m in TRACE.finditer(stderr):
        out[m.groups()] = out.get(m.groups(), 0) + 1
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = {}
    for tag, mode, nproc, env in (
            ("fused", "all", 2, {**ENV, "UCC_TL_CDNA4_ZC_FUSED": "1"}),
            ("three_kernel", "all", 2, {**ENV, "UCC_TL_CDNA4_ZC_FUSED": "0"}),
            ("ranks3", "three", 3, {**ENV, "UCC_TL_CDNA4_ZC_FUSED": "1"}),
            ("trig", "trig", 2, dict(ENV)),
            ("off", "off", 2, {k: v for k, v in ENV.items()
                               if k != "UCC_TL_CDNA4_GATED_ROOTED"})):
        d = tmp_path_factory.mktemp(tag)
        saved = os.environ.pop("UCC_TL_CDNA4_GATED_ROOTED", None)
        try:
            proc = _torchrun([WORKER, str(d), mode], timeout=240,
                             env_extra=env, nproc=nproc)
        finally:
            if saved is not None:
                os.environ["UCC_TL_CDNA4_GATED_ROOTED"] = saved
        sys.stdout.write(f"--- {tag}: rc={proc.returncode}\n")
        sys.stdout.write(proc.stdout[-2000:])
        sys.stderr.write("\n".join(
            ln for ln in proc.stderr.splitlines()
            if " DEBUG " not in ln and " INFO " not in ln)[-3000:])
        out[tag] = (proc, str(d))
    return out


def _ok(runs, tag, nproc):
    proc, _ = runs[tag]
    assert proc.returncode == 0
    assert proc.stdout.count("GRT_OK") == nproc
    return proc


@pytest.mark.parametrize("tag", ["fused", "three_kernel"])
def test_two_ranks(runs, tag):
    """Every case of the worker passed its own checks, and every full-team
    bcast and reduce was served by the gated pipeline."""
    proc = _ok(runs, tag, 2)
    ch = rooted_choices(proc.stderr)
    assert ch.get(("bcast", "cdna4/gated_pipeline"), 0) > 0
    assert ch.get(("reduce", "cdna4/gated_pipeline"), 0) > 0
    assert set(alg for _, alg in ch) == {"cdna4/gated_pipeline"}, ch
    # the misaligned persistent bcast fell back to staging by consensus
    assert "zero-copy disabled by team consensus" in proc.stderr


def test_one_kernel_paths(runs):
    fused = _ok(runs, "fused", 2).stderr
    three = _ok(runs, "three_kernel", 2).stderr
    assert BCAST_ONE in fused and REDUCE_ONE in fused
    assert BCAST_THREE not in fused and REDUCE_THREE not in fused
    assert BCAST_ONE not in three and REDUCE_ONE not in three
    assert BCAST_THREE in three and REDUCE_THREE in three


def test_bitwise_equal_between_runs(runs):
    _ok(runs, "fused", 2)
    _ok(runs, "three_kernel", 2)
    d1, d0 = runs["fused"][1], runs["three_kernel"][1]
    names = sorted(os.path.basename(p)
                   for p in glob.glob(os.path.join(d1, "*.npy")))
    assert names == sorted(os.path.basename(p)
                           for p in glob.glob(os.path.join(d0, "*.npy")))
    # per root: 6 bcast + 9 reduce cases; 6 interleave steps; 2 ranks
    assert len(names) == 2 * (2 * 15 + 6), len(names)
    for n in names:
        a = np.load(os.path.join(d1, n))
        b = np.load(os.path.join(d0, n))
        assert a.shape == b.shape, n
        assert np.array_equal(a, b), n


def test_three_ranks(runs):
    proc = _ok(runs, "ranks3", 3)
    ch = rooted_choices(proc.stderr)
    assert set(alg for _, alg in ch) == {"cdna4/gated_pipeline"}, ch
    assert BCAST_ONE in proc.stderr and REDUCE_ONE in proc.stderr


def test_triggered(runs):
    proc = _ok(runs, "trig", 2)
    ch = rooted_choices(proc.stderr)
    assert set(alg for _, alg in ch) == {"cdna4/gated_pipeline"}, ch
    # triggered posts of the rooted types never run a zero-copy pattern
    for path in (BCAST_ONE, BCAST_THREE, REDUCE_ONE, REDUCE_THREE):
        assert path not in proc.stderr


def test_knob_off(runs):
    proc = _ok(runs, "off", 2)
    ch = rooted_choices(proc.stderr)
    assert ch.get(("bcast", "cdna4/staged_linear"), 0) > 0
    assert ch.get(("reduce", "cdna4/staged_linear"), 0) > 0
    assert set(alg for _, alg in ch) == {"cdna4/staged_linear"}, ch
