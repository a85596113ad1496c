"""Grid size and cache policy of tl/cdna4's gated collectives
(src/tl/cdna4/zc_policy.h) with no GPU: tests/native/test_zc_policy.cc
tabulates the rule over collective x path x n in {2, 3, 4, 8} x depth in
{1, 2, 4} x sizes around 64, 128, 160 and at 256 MiB x the GATED_BLOCKS and
ZC_STREAM overrides, against the grid rule as tl_cdna4.cc stated it and
the one case in which streaming is on.

The program is a host-only translation unit with its own main, so it is
compiled here, once plainly and once with the address and undefined
behaviour sanitizers, by whichever host C++ compiler is present."""

import os
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "test_zc_policy.cc")


def _compiler():
    # clang first: it links the sanitizer runtimes statically
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
    assert cc.returncode == 0, "test_zc_policy.cc does not compile"
    env = dict(os.environ)
    env.update(env_extra or {})
    p = subprocess.run([binary], capture_output=True, text=True,
                       timeout=300, env=env)
    sys.stdout.write(p.stdout[-2000:])
    sys.stderr.write(p.stderr[-3000:])
    return p


def test_zc_policy_native(tmp_path):
    p = _build_and_run(tmp_path, "test_zc_policy", ["-O2"])
    assert p.returncode == 0
    assert "ZC_POLICY_OK" in p.stdout
    assert "MISMATCH" not in p.stdout


def test_zc_policy_native_sanitized(tmp_path):
    """The same program under -fsanitize=address,undefined: no report."""
    p = _build_and_run(
        tmp_path, "test_zc_policy_san",
        ["-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
        env_extra={"UBSAN_OPTIONS": "print_stacktrace=1"})
    assert p.returncode == 0
    assert "ZC_POLICY_OK" in p.stdout
    assert "runtime error" not in p.stderr
    assert "AddressSanitizer" not in p.stderr


def test_zc_policy_make_target():
    """`make` builds the same program as build/test_zc_policy."""
    binary = os.path.join(REPO, "build", "test_zc_policy")
    assert os.path.exists(binary), "build/test_zc_policy not built (make)"
    p = subprocess.run([binary], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0
    assert "ZC_POLICY_OK" in p.stdout


def test_stream_knob_listed_by_info():
    """`ucc_info -c` shows the knob with its default."""
    info = os.path.join(REPO, "build", "ucc_info")
    assert os.path.exists(info), "build/ucc_info not built (make)"
    env = dict(os.environ)
    env.pop("UCC_TL_CDNA4_ZC_STREAM", None)
    p = subprocess.run([info, "-c"], capture_output=True, text=True,
                       timeout=120, env=env, cwd=REPO)
    assert p.returncode == 0, p.stderr[-500:]
    assert "UCC_TL_CDNA4_ZC_STREAM=auto" in p.stdout
