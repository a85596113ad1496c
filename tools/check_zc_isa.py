#!/usr/bin/env python3
"""Check the compiled resource usage of the fused zero-copy allreduce.

Reads the -Rpass-analysis=kernel-resource-usage remarks of
src/ec/kernels/ec_gated.hip (file argument or stdin; `make check-isa`
produces them) and fails unless

 1. no k_zc_allreduce instantiation uses scratch memory (the kernel
    argument struct and the pack buffers stay in registers:
    docs/GATED_PIPELINE.md "Data phase and its probe");
 2. the flagship k_zc_allreduce<bf16,SUM,8,4> keeps 3 waves/SIMD, in its
    plain and in its streamed (non-temporal) instantiation;
 3. every depth-4 instantiation keeps at least 2 waves/SIMD, i.e. 2
    blocks of 256 threads per CU: the residency arithmetic behind the
    192-block grid in src/tl/cdna4/zc_policy.h.

A kernel is keyed (type, op, vec, depth, streamed). The last template
parameter is the cache policy; a name without it (the kernel before the
policy existed) reads as plain. A k_zc_allreduce name that does not parse
is an error: a changed template list must not empty the checks.

The unit also holds the one-kernel zero-copy bcast:

 4. k_zc_bcast (not a template: one instantiation) uses no scratch memory
    either.

Occupancy is the compiler's figure, VGPRs and AGPRs together."""

import re
import sys

KERNEL = "k_zc_allreduceI"
NAME = re.compile(
    r"k_zc_allreduceI(.+?)Li(\d+)ELi(\d+)ELi(\d+)E(?:Lb([01])E)?EEv")
FLAGSHIP = ("NS0_6bf16_tE", 0, 8, 4, False)
FLAGSHIP_NT = FLAGSHIP[:4] + (True,)
BCAST = re.compile(r"10k_zc_bcastE")


def parse(text):
    out = {}
    for blk in re.split(r"(?=remark: [^\n]*Function Name: )", text):
        m = re.search(r"Function Name: (\S+)", blk)
        if not m or KERNEL not in m.group(1):
            continue
        n = NAME.search(m.group(1))
        if not n:
            raise ValueError("unparsed k_zc_allreduce name: " + m.group(1))

        def field(key):
            return int(re.search(key + r": (\d+)", blk).group(1))

        key = (n.group(1), int(n.group(2)), int(n.group(3)),
               int(n.group(4)), n.group(5) == "1")
        out[key] = dict(vgprs=field("VGPRs"), agprs=field("AGPRs"),
                        scratch=field(r"ScratchSize \[bytes/lane\]"),
                        waves=field(r"Occupancy \[waves/SIMD\]"))
    return out


def parse_bcast(text):
    """ScratchSize of every k_zc_bcast remark block (one is expected)."""
    out = []
    for blk in re.split(r"(?=remark: [^\n]*Function Name: )", text):
        m = re.search(r"Function Name: (\S+)", blk)
        if m and BCAST.search(m.group(1)):
            out.append(int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)",
                                     blk).group(1)))
    return out


def check_bcast(scratch):
    if not scratch:
        return ["k_zc_bcast not found"]
    return [f"k_zc_bcast: {s} B/lane of scratch" for s in scratch if s]


def check(kernels):
    bad = []
    if FLAGSHIP not in kernels:
        return ["flagship k_zc_allreduce<bf16,0,8,4> not found "
                f"({len(kernels)} instantiations parsed)"]
    for key, k in sorted(kernels.items()):
        if k["scratch"]:
            bad.append(f"{key}: {k['scratch']} B/lane of scratch")
        if key[3] == 4 and k["waves"] < 2:
            bad.append(f"{key}: {k['waves']} waves/SIMD at depth 4 "
                       f"({k['vgprs']} VGPRs + {k['agprs']} AGPRs)")
    streamed = any(key[4] for key in kernels)
    if streamed and FLAGSHIP_NT not in kernels:
        bad.append("streamed flagship k_zc_allreduce<bf16,0,8,4,true> "
                   "not found")
    for name, key in (("flagship", FLAGSHIP),
                      ("streamed flagship", FLAGSHIP_NT)):
        f = kernels.get(key)
        if f and f["waves"] < 3:
            bad.append(f"{name}: {f['waves']} waves/SIMD "
                       f"({f['vgprs']} VGPRs + {f['agprs']} AGPRs), want 3")
    return bad


def main():
    text = open(sys.argv[1]).read() if len(sys.argv) > 1 else sys.stdin.read()
    try:
        kernels = parse(text)
    except ValueError as e:
        print("check_zc_isa:", e)
        return 1
    bad = check(kernels) + check_bcast(parse_bcast(text))
    for b in bad:
        print("check_zc_isa:", b)
    if bad:
        return 1
    f = kernels[FLAGSHIP]
    low = min(k["waves"] for key, k in kernels.items() if key[3] == 4)
    nt = sum(1 for key in kernels if key[4])
    g = kernels.get(FLAGSHIP_NT)
    print(f"check_zc_isa ok: {len(kernels)} k_zc_allreduce instantiations "
          f"({nt} streamed), no scratch; flagship {f['vgprs']} VGPRs, "
          f"{f['waves']} waves/SIMD"
          + (f", streamed {g['vgprs']} VGPRs, {g['waves']} waves/SIMD"
             if g else "")
          + f"; depth 4 at least {low} waves/SIMD; k_zc_bcast no scratch")
    return 0


if __name__ == "__main__":
    sys.exit(main())
