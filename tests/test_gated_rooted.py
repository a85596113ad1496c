"""CPU-side checks of the gated bcast / reduce feature: the opt-in knob is
declared with its default, and tools/check_zc_isa.py reads the k_zc_bcast
resource-usage remark."""

import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

sys.path.insert(0, os.path.join(REPO, "tools"))

import check_zc_isa  # noqa: E402


def test_knob_listed_by_info():
    """`ucc_info -c` shows UCC_TL_CDNA4_GATED_ROOTED with its default 0."""
    info = os.path.join(REPO, "build", "ucc_info")
    assert os.path.exists(info), "build/ucc_info not built (make)"
    env = dict(os.environ)
    env.pop("UCC_TL_CDNA4_GATED_ROOTED", None)
    p = subprocess.run([info, "-c"], capture_output=True, text=True,
                       timeout=120, env=env, cwd=REPO)
    assert p.returncode == 0, p.stderr[-500:]
    assert "UCC_TL_CDNA4_GATED_ROOTED=0" in p.stdout


def _remark(name, scratch):
    pre = "src/ec/kernels/ec_gated.hip:1:1: remark: "
    return "".join(pre + ln + " [-Rpass-analysis=kernel-resource-usage]\n"
                   for ln in (f"Function Name: {name}", "    VGPRs: 104",
                              "    AGPRs: 0",
                              f"    ScratchSize [bytes/lane]: {scratch}",
                              "    Occupancy [waves/SIMD]: 4"))


def test_isa_check_reads_zc_bcast():
    name = "_ZN3ucc6ec_hip10k_zc_bcastENS0_9GatedArgsE"
    other = "_ZN3ucc6ec_hip12k_bcast_dataENS0_9GatedArgsE"
    assert check_zc_isa.check_bcast(check_zc_isa.parse_bcast(
        _remark(other, 8) + _remark(name, 0))) == []
    bad = check_zc_isa.check_bcast(check_zc_isa.parse_bcast(
        _remark(name, 24)))
    assert len(bad) == 1 and "24 B/lane" in bad[0]
    assert check_zc_isa.check_bcast(check_zc_isa.parse_bcast(
        _remark(other, 0))) == ["k_zc_bcast not found"]
