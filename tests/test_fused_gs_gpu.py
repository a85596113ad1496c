"""The fused one-kernel gather / scatter / gatherv / scatterv of tl/cdna4
(UCC_TL_CDNA4_FUSED_GATHER_SCATTER=1): tests/fused_gs_worker.py runs seeded
exact-integer cases and compares every destination bit for bit. Four
torchrun launches in total (ranks share cuda:0), shared by all tests of this
file; the worker's docstring lists the modes.

Selection is read from the UCC_COLL_TRACE lines: every rank writes down for
every request of the four types whether it must trace cdna4/fused, and the
multiset of trace lines must match. Which kernel served a post is read from
the debug lines, one per post: k_fused_coll, k_fused_coll_graph or
k_fused_rooted_v, and for a gatherv or scatterv that the root found too
large the fallback line."""

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
WORKER = os.path.join(REPO, "tests", "fused_gs_worker.py")

HOST_KERNEL = re.compile(
    r"cdna4 fused (gather|scatter): host-sequenced kernel \(k_fused_coll\)")
GRAPH_KERNEL = re.compile(
    r"cdna4 fused (gather|scatter): graph kernel \(k_fused_coll_graph\)")
ROOTED_KERNEL = re.compile(
    r"cdna4 fused (gatherv|scatterv): host-sequenced kernel "
    r"\(k_fused_rooted_v\), (\d+) blocks, bound (\d+) bytes")
FALLBACK = re.compile(
    r"cdna4 fused (gatherv|scatterv): the counts exceed the (\d+)-byte "
    r"bound, served by (\w+)")
FOUR = ("gather", "scatter", "gatherv", "scatterv")
B = 524288 - 144

ENV = {
    "UCC_TL_CDNA4_FUSED_GATHER_SCATTER": "1",
    "UCC_TL_CDNA4_FUSED_COLLS_MAX": "524288",
    "UCC_COLL_TRACE": "1",
    "UCC_LOG_LEVEL": "debug",
}
ENV_OFF = {"UCC_COLL_TRACE": "1", "UCC_LOG_LEVEL": "debug"}

TRACE = re.compile(r"coll (\w+) mem \w+ size (\d+) -> (\w+)/(\w+) ")
REQ = re.compile(r"^FG_REQ (\w+) (\d+) ([FO])$", re.M)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    saved = os.environ.pop("UCC_TL_CDNA4_FUSED_GATHER_SCATTER", None)
    out = {}
    try:
        for mode, nproc, env in (("all", 2, ENV), ("three", 3, ENV),
                                 ("trig", 2, ENV), ("off", 2, ENV_OFF)):
            d = tmp_path_factory.mktemp(mode)
            proc = _torchrun([WORKER, str(d), mode], timeout=240,
                             env_extra=env, nproc=nproc)
            proc.notes = "".join(
                open(f).read() for f in
                sorted(glob.glob(os.path.join(str(d), "*.txt"))))
            sys.stdout.write(f"--- {mode}: rc={proc.returncode}\n")
            sys.stdout.write(proc.stdout[-1500:])
            sys.stderr.write("\n".join(
                ln for ln in proc.stderr.splitlines()
                if " DEBUG " not in ln and " INFO " not in ln)[-3000:])
            out[mode] = proc
    finally:
        if saved is not None:
            os.environ["UCC_TL_CDNA4_FUSED_GATHER_SCATTER"] = saved
    return out


def _traced(proc):
    """(coll, msgsize, traced cdna4/fused) of every trace line of the four
    types."""
    got = collections.Counter()
    for coll, size, tl, alg in TRACE.findall(proc.stderr):
        if coll in FOUR:
            got[(coll, int(size), (tl, alg) == ("cdna4", "fused"))] += 1
    return got


def _announced(proc):
    return collections.Counter(
        (coll, int(size), f == "F")
        for coll, size, f in REQ.findall(proc.notes))


def _ok(proc, nranks):
    assert proc.returncode == 0
    assert proc.stdout.count("FG_OK") == nranks


def _sum(proc, key):
    return sum(int(x) for x in
               re.findall(r"^FG_%s (\d+)$" % key, proc.notes, re.M))


@pytest.mark.parametrize("mode,nranks", [("all", 2), ("three", 3)])
def test_results_and_selection(runs, mode, nranks):
    """Every case is bitwise right, gaps and bands intact, a non-root's dst
    of gather(v) untouched (asserted in the worker). Every in-bound gather
    and scatter and every gatherv and scatterv traced cdna4/fused, every
    gather and scatter over the bound something else. One kernel line per
    post, of the expected kernel. Every post with a block over B, or a sum
    over it, fell back on every rank, also on a rank whose own count is
    small."""
    proc = runs[mode]
    _ok(proc, nranks)
    want = _announced(proc)
    assert want == _traced(proc)
    for coll in FOUR:
        assert any(f for (c, _, f) in want if c == coll), coll
    for coll in ("gather", "scatter"):
        assert any(not f for (c, _, f) in want if c == coll), coll
        # over the bound: staged_linear, as with the knob unset
        assert {alg for c, s, tl, alg in TRACE.findall(proc.stderr)
                if c == coll and (tl, alg) != ("cdna4", "fused")} == \
            {"staged_linear"}
    assert len(HOST_KERNEL.findall(proc.stderr)) == _sum(proc, "COLL") > 0
    assert not GRAPH_KERNEL.search(proc.stderr)
    rooted = ROOTED_KERNEL.findall(proc.stderr)
    assert len(rooted) == _sum(proc, "ROOTED") > 0
    assert {c for c, _, _ in rooted} == {"gatherv", "scatterv"}
    # B is the same on every rank and post; the requests with 75 001
    # elements or more ran on more than one block
    assert {b for _, _, b in rooted} == {str(B)}
    assert min(int(g) for _, g, _ in rooted) == 1
    assert max(int(g) for _, g, _ in rooted) > 1
    fell = FALLBACK.findall(proc.stderr)
    # one line per rank and post: the same number on every rank
    assert len(fell) == _sum(proc, "FALLBACK") > 0
    assert len(fell) % nranks == 0
    per_rank = collections.Counter(
        re.findall(r"^FG_FALLBACK (\d+)$", proc.notes, re.M))
    assert len(per_rank) == 1
    assert {(b, alg) for _, b, alg in fell} == {(str(B), "staged_linear")}
    assert {c for c, _, _ in fell} == {"gatherv", "scatterv"}


def test_triggered_and_graph_replay(runs):
    proc = runs["trig"]
    _ok(proc, 2)
    want = _announced(proc)
    assert want == _traced(proc)
    assert all(f for (_, _, f) in want)
    # 2 gathers, 2 scatters and the gatherv, on 2 ranks
    assert sum(want.values()) == 2 * 5
    # three eager posts and one capture per request, none host-sequenced;
    # the gatherv's triggered post launched nothing of its own
    assert len(GRAPH_KERNEL.findall(proc.stderr)) == _sum(proc, "GRAPH") \
        == 2 * 4 * 4
    assert not HOST_KERNEL.search(proc.stderr)
    assert "k_fused_rooted_v" not in proc.stderr
    assert not FALLBACK.search(proc.stderr)


def test_knob_unset_keeps_selection(runs):
    proc = runs["off"]
    _ok(proc, 2)
    got = _traced(proc)
    assert got == _announced(proc)
    assert sum(got.values()) == 2 * len(FOUR)
    algs = {coll: alg for coll, _, _, alg in TRACE.findall(proc.stderr)
            if coll in FOUR}
    assert algs == dict.fromkeys(FOUR, "staged_linear")
    # the score map printed at team creation has no fused entry for them
    assert not re.search(r"^(%s):\w+:\S*@cdna4/fused" % "|".join(FOUR),
                         proc.stderr, re.M)
    assert "gatherv:cuda:" in proc.stderr
    assert "cdna4 fused" not in proc.stderr
