"""The v-forms of the fused-collective plan (fused_plan_init_v in
src/tl/cdna4/fused_plan.h: allgatherv, reduce_scatterv, alltoallv) with no
GPU: tests/native/test_fused_plan_v.cc simulates every rank on host memory,
n = 2..8, element sizes {1, 2, 4, 8, 16}, in place where legal, seeded
count matrices with zero pairs, a rank that sends nothing, a rank that
receives nothing, blocks of 1 and 7 elements, displacements permuted and
with gaps; for alltoallv also the vote at exactly one cell and at one
element more.

The program is a host-only translation unit with its own main, so it is
compiled here, once plainly and once with the address and undefined
behaviour sanitizers, by whichever host C++ compiler is present."""

import os
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "test_fused_plan_v.cc")


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
    assert cc.returncode == 0, "test_fused_plan_v.cc does not compile"
    env = dict(os.environ)
    env.update(env_extra or {})
    p = subprocess.run([binary], capture_output=True, text=True,
                       timeout=300, env=env)
    sys.stdout.write(p.stdout[-500:])
    sys.stderr.write(p.stderr[-3000:])
    return p


def test_fused_plan_v_native(tmp_path):
    """The result is the collective's definition; every defined dst byte is
    written once, gaps and guard bands never; scratch offsets are multiples
    of 16 and below scratch_bytes; scratch_bytes and the alltoallv cell are
    equal on all ranks; one oversized pair makes every rank's verdict "does
    not fit" and then nothing is read."""
    p = _build_and_run(tmp_path, "test_fused_plan_v", ["-O2"])
    assert p.returncode == 0
    assert "FUSED_PLAN_V_OK" in p.stdout
    assert "FAIL" not in p.stdout


def test_fused_plan_v_native_sanitized(tmp_path):
    """The same program under -fsanitize=address,undefined: no report."""
    p = _build_and_run(
        tmp_path, "test_fused_plan_v_san",
        ["-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
        # leak checking needs ptrace, which not every sandbox grants; the
        # program owns nothing but std::vectors
        env_extra={"ASAN_OPTIONS": "detect_leaks=0",
                   "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert p.returncode == 0
    assert "FUSED_PLAN_V_OK" in p.stdout
    assert "runtime error" not in p.stderr
    assert "AddressSanitizer" not in p.stderr


def test_fused_plan_v_make_target():
    """`make` builds the same program as build/test_fused_plan_v."""
    binary = os.path.join(REPO, "build", "test_fused_plan_v")
    assert os.path.exists(binary), "build/test_fused_plan_v not built (make)"
    p = subprocess.run([binary], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0
    assert "FUSED_PLAN_V_OK" in p.stdout


def test_fused_colls_knob_help_names_the_eight_types():
    """`ucc_info -c` describes the knob with all eight collectives and
    the alltoallv pair bound; with the knob unset the printed score map
    still has no cdna4 fused entry but the allreduce's."""
    info = os.path.join(REPO, "build", "ucc_info")
    assert os.path.exists(info), "build/ucc_info not built (make)"
    env = dict(os.environ)
    for k in ("UCC_TL_CDNA4_FUSED_COLLS", "UCC_TL_CDNA4_FUSED_COLLS_MAX",
              "UCC_TUNE"):
        env.pop(k, None)
    p = subprocess.run([info, "-c", "-s"], capture_output=True,
                       text=True, timeout=120, env=env, cwd=REPO)
    assert p.returncode == 0, p.stderr[-500:]
    text = " ".join(p.stdout.split())
    for coll in ("allgather,", "allgatherv,", "reduce_scatter,",
                 "reduce_scatterv,", "alltoall,", "alltoallv,", "bcast",
                 "reduce "):
        assert coll in text, coll
    assert "(MAX - 16) / n" in text
    for ln in p.stdout.splitlines():
        if "cdna4/fused" in ln:
            assert ln.split(":")[0] == "allreduce", ln
