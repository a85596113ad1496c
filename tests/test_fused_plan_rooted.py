"""The rooted copy collectives of the fused-collective plan
(src/tl/cdna4/fused_plan.h: gather and scatter through fused_plan_init,
gatherv and scatterv through fused_plan_init_rooted_v) with no GPU:
tests/native/test_fused_plan_rooted.cc simulates every rank on host memory,
n = 2..8, every root, element sizes {1, 2, 4, 8, 16}, in place at the root
and not; blocks of 1 element, exactly 16 bytes, 7 and 999 elements; seeded
counts with zeros, a root whose own count is zero, a rank that is the only
non-zero one, displacements permuted and with gaps; a count of exactly the
bound B and of B plus one element at the root's own index and at another
rank's; for scatterv a stride sum of exactly B and of B + 16; a rank whose
own length disagrees with the root's table.

The program is a host-only translation unit with its own main, so it is
compiled here, once plainly and once with the address and undefined
behaviour sanitizers, by whichever host C++ compiler is present."""

import os
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "test_fused_plan_rooted.cc")
FOUR = ("gather", "scatter", "gatherv", "scatterv")


def _compiler():
    # clang first: it links the sanitizer runtimes statically, so the
    # sanitized program does not care what else the loader brings in
    for cxx in (os.environ.get("CXX"), "clang++",
                "/opt/rocm/llvm/bin/clang++", "g++", "c++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    pytest.fail("no host C++ compiler found")


def _build_and_run(tmp_path, name, flags, env_extra=None):
    binary = str(tmp_path / name)
    cc = subprocess.run(
        [_compiler(), "-std=c++17", "-Wall", "-Wextra", *flags, SRC, "-o",
         binary], capture_output=True, text=True, timeout=300)
    sys.stderr.write(cc.stderr[-3000:])
    assert cc.returncode == 0, "test_fused_plan_rooted.cc does not compile"
    env = dict(os.environ)
    env.update(env_extra or {})
    p = subprocess.run([binary], capture_output=True, text=True,
                       timeout=300, env=env)
    sys.stdout.write(p.stdout[-500:])
    sys.stderr.write(p.stderr[-3000:])
    return p


def test_fused_plan_rooted_native(tmp_path):
    """The result is the collective's definition; every defined dst byte is
    written once; gaps, guard bands, the root's in-place block and every
    non-root dst of gather(v) never; scratch offsets are multiples of 16 and
    below scratch_bytes; scratch_bytes and B are equal on all ranks; a "does
    not fit" verdict reads and writes nothing; a rank whose length disagrees
    with the table copies the smaller one and stays inside its dst."""
    p = _build_and_run(tmp_path, "test_fused_plan_rooted", ["-O2"])
    assert p.returncode == 0
    assert "FUSED_PLAN_ROOTED_OK" in p.stdout
    assert "FAIL" not in p.stdout


def test_fused_plan_rooted_native_sanitized(tmp_path):
    """The same program under -fsanitize=address,undefined: no report."""
    p = _build_and_run(
        tmp_path, "test_fused_plan_rooted_san",
        ["-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
        # leak checking needs ptrace, which not every sandbox grants; the
        # program owns nothing but std::vectors
        env_extra={"ASAN_OPTIONS": "detect_leaks=0",
                   "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert p.returncode == 0
    assert "FUSED_PLAN_ROOTED_OK" in p.stdout
    assert "runtime error" not in p.stderr
    assert "AddressSanitizer" not in p.stderr


def test_fused_plan_rooted_make_target():
    """`make` builds the same program as build/test_fused_plan_rooted."""
    binary = os.path.join(REPO, "build", "test_fused_plan_rooted")
    assert os.path.exists(binary), \
        "build/test_fused_plan_rooted not built (make)"
    p = subprocess.run([binary], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0
    assert "FUSED_PLAN_ROOTED_OK" in p.stdout


def _ucc_info(extra_env=None):
    info = os.path.join(REPO, "build", "ucc_info")
    assert os.path.exists(info), "build/ucc_info not built (make)"
    env = dict(os.environ)
    for k in ("UCC_TL_CDNA4_FUSED_COLLS", "UCC_TL_CDNA4_FUSED_COLLS_MAX",
              "UCC_TL_CDNA4_FUSED_GATHER_SCATTER", "UCC_TUNE"):
        env.pop(k, None)
    env.update(extra_env or {})
    p = subprocess.run([info, "-c", "-s"], capture_output=True,
                       text=True, timeout=120, env=env, cwd=REPO)
    assert p.returncode == 0, p.stderr[-500:]
    return p.stdout


def test_fused_gather_scatter_knob_help_and_default():
    """`ucc_info -c` shows the knob, default 0, with a help text of its own
    that names the four types and both bounds; with the knob unset the
    printed score map has no cdna4 fused entry for them."""
    out = _ucc_info()
    lines = out.splitlines()
    at = [i for i, ln in enumerate(lines)
          if "UCC_TL_CDNA4_FUSED_GATHER_SCATTER" in ln]
    assert len(at) == 1, at
    assert re_default(lines[at[0]]) == "0", lines[at[0]]
    # the help text: the comment lines next to the knob's own line
    text = " ".join(out.split())
    start = text.index("serve small full-team device gather,")
    helptext = text[start:text.index("must be the same on every rank",
                                     start)]
    for coll in ("gather,", "scatter,", "gatherv", "scatterv"):
        assert coll in helptext, coll
    assert "MAX - 144" in helptext
    assert "largest block is at most B" in helptext
    assert "sum of the blocks" in helptext
    assert "staged_linear" in helptext
    # the score map lists cdna4 only where there is a device; whichever
    # entries the four types have, none is fused
    seen = set()
    for ln in lines:
        coll = ln.split(":")[0]
        if coll in FOUR:
            seen.add(coll)
            assert "cdna4/fused" not in ln, ln
    assert seen == set(FOUR)


def re_default(line):
    """The value of a `NAME=value` line of `ucc_info -c`."""
    return line.split("=", 1)[1].split()[0]
