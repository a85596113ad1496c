"""tools/check_zc_isa.py on synthetic kernel-resource-usage remarks: names
with and without the cache-policy template parameter are parsed, the
checks cover the streamed instantiations, and a k_zc_allreduce name that
does not parse is an error instead of a silently shorter list."""

import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import check_zc_isa  # noqa: E402

BF16 = "NS0_6bf16_tE"


def remark(name, vgprs=159, agprs=0, scratch=0, waves=3):
    loc = "src/ec/kernels/ec_gated.hip:660:1: remark: "
    tail = " [-Rpass-analysis=kernel-resource-usage]\n"
    return "".join(loc + ln + tail for ln in (
        f"Function Name: {name}", "    TotalSGPRs: 70",
        f"    VGPRs: {vgprs}", f"    AGPRs: {agprs}",
        f"    ScratchSize [bytes/lane]: {scratch}",
        "    Dynamic Stack: False",
        f"    Occupancy [waves/SIMD]: {waves}", "    SGPRs Spill: 0",
        "    VGPRs Spill: 0", "    LDS Size [bytes/block]: 8"))


def zc(t=BF16, op=0, vec=8, depth=4, nt=None):
    policy = "" if nt is None else f"Lb{int(nt)}E"
    return (f"_ZN3ucc6ec_hip14k_zc_allreduceI{t}Li{op}ELi{vec}ELi{depth}E"
            f"{policy}EEvNS0_9GatedArgsE")


def test_names_with_and_without_policy():
    text = (remark(zc(nt=False)) + remark(zc(nt=True)) +
            remark(zc(t="fE", vec=4, depth=2, nt=False), vgprs=120) +
            remark("_ZN3ucc6ec_hip14k_staged_stageENS0_9GatedArgsE"))
    k = check_zc_isa.parse(text)
    assert set(k) == {(BF16, 0, 8, 4, False), (BF16, 0, 8, 4, True),
                      ("fE", 0, 4, 2, False)}
    assert check_zc_isa.check(k) == []
    # the kernel before the policy parameter existed reads as plain
    old = check_zc_isa.parse(remark(zc()) + remark(zc(depth=1), vgprs=34,
                                                    waves=8))
    assert set(old) == {(BF16, 0, 8, 4, False), (BF16, 0, 8, 1, False)}
    assert check_zc_isa.check(old) == []


def test_streamed_with_scratch_is_reported():
    k = check_zc_isa.parse(remark(zc(nt=False)) + remark(zc(nt=True)) +
                           remark(zc(op=1, nt=True), scratch=16))
    bad = check_zc_isa.check(k)
    assert len(bad) == 1 and "16 B/lane of scratch" in bad[0]
    assert "True" in bad[0]


def test_streamed_below_two_waves_at_depth_4_is_reported():
    k = check_zc_isa.parse(
        remark(zc(nt=False)) + remark(zc(nt=True)) +
        remark(zc(t="aE", vec=16, nt=True), vgprs=256, agprs=40, waves=1))
    bad = check_zc_isa.check(k)
    assert len(bad) == 1 and "1 waves/SIMD at depth 4" in bad[0]


def test_streamed_flagship_needs_three_waves():
    k = check_zc_isa.parse(remark(zc(nt=False)) +
                           remark(zc(nt=True), vgprs=188, waves=2))
    bad = check_zc_isa.check(k)
    assert len(bad) == 1 and bad[0].startswith("streamed flagship: 2 waves")
    # streamed instantiations without the streamed flagship
    k = check_zc_isa.parse(remark(zc(nt=False)) + remark(zc(op=1, nt=True)))
    assert any("streamed flagship" in b and "not found" in b
               for b in check_zc_isa.check(k))


def test_unparsed_name_is_an_error():
    odd = "_ZN3ucc6ec_hip14k_zc_allreduceINS0_6bf16_tELi0ELi8EEEvNS0_9GatedArgsE"
    with pytest.raises(ValueError, match="unparsed k_zc_allreduce name"):
        check_zc_isa.parse(remark(zc(nt=False)) + remark(odd))


def test_main_fails_on_unparsed_name(tmp_path, capsys, monkeypatch):
    odd = "_ZN3ucc6ec_hip14k_zc_allreduceIfLi0ELi4ELi4ELc1EEEvNS0_9GatedArgsE"
    f = tmp_path / "remarks.txt"
    f.write_text(remark(zc(nt=False)) + remark(odd))
    monkeypatch.setattr(sys, "argv", ["check_zc_isa.py", str(f)])
    assert check_zc_isa.main() == 1
    assert "unparsed k_zc_allreduce name" in capsys.readouterr().out
