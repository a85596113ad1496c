"""The schedule of tl/cdna4's multi-ring collectives
(src/tl/cdna4/ring_plan.h) with no GPU: tests/native/test_ring_plan.cc
simulates every rank on host memory, n = 2..8, every ring count, the three
collectives, in randomised launch orders that respect the gate, and shows
that the gate's right-neighbour clause is needed.

The program is a host-only translation unit with its own main, so it is
compiled here, once plainly and once with the address and undefined
behaviour sanitizers, by whichever host C++ compiler is present."""

import os
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "test_ring_plan.cc")


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
    assert cc.returncode == 0, "test_ring_plan.cc does not compile"
    env = dict(os.environ)
    env.update(env_extra or {})
    p = subprocess.run([binary], capture_output=True, text=True,
                       timeout=300, env=env)
    sys.stdout.write(p.stdout[-500:])
    sys.stderr.write(p.stderr[-3000:])
    return p


def test_ring_plan_native(tmp_path):
    """Every block gets every rank's contribution exactly once, final
    placement is right, no outbox half is overwritten before its reader's
    launch; without the right-neighbour clause an overwrite is reported."""
    p = _build_and_run(tmp_path, "test_ring_plan", ["-O2"])
    assert p.returncode == 0
    assert "RING_PLAN_OK" in p.stdout
    assert "gate_hits=0 " not in p.stdout


def test_ring_plan_native_sanitized(tmp_path):
    """The same program under -fsanitize=address,undefined: no report."""
    p = _build_and_run(
        tmp_path, "test_ring_plan_san",
        ["-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
        # leak checking needs ptrace, which not every sandbox grants; the
        # program owns nothing but std::vectors
        env_extra={"ASAN_OPTIONS": "detect_leaks=0",
                   "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert p.returncode == 0
    assert "RING_PLAN_OK" in p.stdout
    assert "runtime error" not in p.stderr
    assert "AddressSanitizer" not in p.stderr


def test_ring_plan_make_target():
    """`make` builds the same program as build/test_ring_plan."""
    binary = os.path.join(REPO, "build", "test_ring_plan")
    assert os.path.exists(binary), "build/test_ring_plan not built (make)"
    p = subprocess.run([binary], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0
    assert "RING_PLAN_OK" in p.stdout


def test_ring_knobs_listed_by_info():
    """`ucc_info -c` shows the two ring knobs with their defaults; with no
    GPU (and with the knob unset) the printed score map has no cdna4 ring."""
    info = os.path.join(REPO, "build", "ucc_info")
    assert os.path.exists(info), "build/ucc_info not built (make)"
    env = dict(os.environ)
    for k in ("UCC_TL_CDNA4_RING", "UCC_TL_CDNA4_RING_NRINGS", "UCC_TUNE"):
        env.pop(k, None)
    p = subprocess.run([info, "-c", "-s"], capture_output=True, text=True,
                       timeout=120, env=env, cwd=REPO)
    assert p.returncode == 0, p.stderr[-500:]
    assert "UCC_TL_CDNA4_RING=0" in p.stdout
    assert "UCC_TL_CDNA4_RING_NRINGS=0" in p.stdout
    assert "cdna4/ring" not in p.stdout
