/* Host-only table check of src/tl/cdna4/zc_policy.h: grid size and cache
 * policy of the gated collectives over collective x path x n x depth x
 * size x single-fragment x GATED_BLOCKS x ZC_STREAM.
 *
 * The expected grid is the rule as tl_cdna4.cc stated it before it moved
 * into the header, written out once more below in its own words:
 *   64 blocks by default; 128 from 160 MiB up for a single fragment; 192
 *   from 128 MiB up for the one-kernel allreduce of 2 ranks at depth 4;
 *   UCC_TL_CDNA4_GATED_BLOCKS, when set, wins over all of them.
 * The expected policy: streaming in that last case only; knob 0 never;
 * knob 1 wherever k_zc_allreduce has a streamed instantiation (one-kernel
 * allreduce, reduce_scatter or rooted reduce at depth 4), at any size.
 * The table compares against that rule restated; what does not lean on a
 * restatement are the counts of streamed cases, worked out by hand from
 * the table's axes, and the spot list, spelled out value by value. */
#include <cstdint>
#include <cstdio>

#include "../../src/tl/cdna4/zc_policy.h"

using namespace ucc::tl_cdna4;

static int expect_blocks(ZcColl ct, bool one_kernel, int n, int depth,
                         uint64_t total, bool single, int ov)
{
    if (ov > 0) { /* 0 = unset; the TL clamps negatives to 0, and the
                   * rule ignores them too */
        return ov;
    }
    if (one_kernel && ct == ZC_COLL_ALLREDUCE && n == 2 && depth == 4 &&
        total >= (uint64_t)128 << 20) {
        return 192;
    }
    if (single && total >= (uint64_t)160 << 20) {
        return 128;
    }
    return 64;
}

static bool expect_stream(ZcColl ct, bool one_kernel, int n, int depth,
                          uint64_t total, int knob)
{
    if (knob == 0 || !one_kernel || depth != 4) {
        return false;
    }
    if (knob == 1) {
        return ct == ZC_COLL_ALLREDUCE || ct == ZC_COLL_REDUCE_SCATTER ||
               ct == ZC_COLL_REDUCE;
    }
    return ct == ZC_COLL_ALLREDUCE && n == 2 &&
           total >= (uint64_t)128 << 20;
}

int main()
{
    const ZcColl   colls[]  = {ZC_COLL_ALLREDUCE, ZC_COLL_REDUCE_SCATTER,
                               ZC_COLL_REDUCE, ZC_COLL_BCAST, ZC_COLL_OTHER};
    const int      ns[]     = {2, 3, 4, 8};
    const int      depths[] = {1, 2, 4};
    const uint64_t M        = 1024 * 1024;
    const uint64_t sizes[]  = {64 * M - 1,  64 * M,      128 * M - 1, 128 * M,
                               160 * M - 1, 160 * M,     256 * M};
    const int      ovs[]    = {0, -1, 8, 256};
    const int      knobs[]  = {ZC_STREAM_AUTO, ZC_STREAM_OFF, ZC_STREAM_ON};
    long           cases = 0, bad = 0, streamed_auto = 0, streamed_on = 0;
    for (ZcColl ct : colls) {
        for (int one = 0; one < 2; one++) {
            for (int n : ns) {
                for (int d : depths) {
                    for (uint64_t sz : sizes) {
                        for (int single = 0; single < 2; single++) {
                            /* the one-kernel path runs one fragment */
                            if (one && !single) {
                                continue;
                            }
                            for (int ov : ovs) {
                                for (int kb : knobs) {
                                    const ZcPolicy p = zc_policy(
                                        ct, one != 0, n, d, sz, single != 0,
                                        ov, kb);
                                    const int  eb = expect_blocks(
                                        ct, one != 0, n, d, sz, single != 0,
                                        ov);
                                    const bool es = expect_stream(
                                        ct, one != 0, n, d, sz, kb);
                                    cases++;
                                    streamed_auto +=
                                        kb == ZC_STREAM_AUTO && p.stream;
                                    streamed_on +=
                                        kb == ZC_STREAM_ON && p.stream;
                                    if (kb == ZC_STREAM_OFF && p.stream) {
                                        bad++;
                                        printf("knob 0 streamed\n");
                                    }
                                    if (p.blocks != eb || p.stream != es) {
                                        bad++;
                                        printf("MISMATCH ct=%d one=%d n=%d "
                                               "d=%d sz=%llu single=%d ov=%d "
                                               "knob=%d: blocks %d want %d, "
                                               "stream %d want %d\n",
                                               (int)ct, one, n, d,
                                               (unsigned long long)sz,
                                               single, ov, kb, p.blocks, eb,
                                               (int)p.stream, (int)es);
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }
    }
    /* spot values, spelled out: the flagship and its neighbours */
    struct Spot {
        ZcColl   ct;
        bool     one;
        int      n, d;
        uint64_t sz;
        int      ov, knob, blocks;
        bool     stream;
        bool     single = true;
    } const spots[] = {
        {ZC_COLL_ALLREDUCE, true, 2, 4, 256 * M, 0, ZC_STREAM_AUTO, 192, true},
        {ZC_COLL_ALLREDUCE, true, 2, 4, 128 * M, 0, ZC_STREAM_AUTO, 192, true},
        {ZC_COLL_ALLREDUCE, true, 2, 4, 128 * M - 1, 0, ZC_STREAM_AUTO, 64,
         false},
        {ZC_COLL_ALLREDUCE, true, 2, 4, 256 * M, 0, ZC_STREAM_OFF, 192, false},
        {ZC_COLL_ALLREDUCE, true, 2, 4, 256 * M, 256, ZC_STREAM_AUTO, 256,
         true},
        {ZC_COLL_ALLREDUCE, true, 2, 4, 4096, 8, ZC_STREAM_ON, 8, true},
        {ZC_COLL_ALLREDUCE, true, 2, 2, 256 * M, 0, ZC_STREAM_ON, 128, false},
        {ZC_COLL_ALLREDUCE, true, 4, 2, 256 * M, 0, ZC_STREAM_ON, 128, false},
        {ZC_COLL_ALLREDUCE, false, 2, 4, 256 * M, 0, ZC_STREAM_ON, 128, false},
        {ZC_COLL_REDUCE_SCATTER, true, 2, 4, 256 * M, 0, ZC_STREAM_AUTO, 128,
         false},
        {ZC_COLL_REDUCE_SCATTER, true, 2, 4, 4096, 0, ZC_STREAM_ON, 64, true},
        {ZC_COLL_REDUCE, true, 2, 4, 256 * M, 0, ZC_STREAM_AUTO, 128, false},
        {ZC_COLL_BCAST, true, 2, 4, 256 * M, 0, ZC_STREAM_ON, 128, false},
        /* 3 and 4 ranks forced to depth 4 (the launcher halves it, so the
         * TL never asks this): the kernel form exists at depth 4, so knob
         * 1 streams; auto does not, and the grid is not the 2-rank one */
        {ZC_COLL_ALLREDUCE, true, 3, 4, 256 * M, 0, ZC_STREAM_ON, 128, true},
        {ZC_COLL_ALLREDUCE, true, 4, 4, 256 * M, 0, ZC_STREAM_ON, 128, true},
        {ZC_COLL_ALLREDUCE, true, 3, 4, 256 * M, 0, ZC_STREAM_AUTO, 128,
         false},
        {ZC_COLL_ALLREDUCE, true, 4, 4, 128 * M, 0, ZC_STREAM_AUTO, 64, false},
        /* several fragments: never the one-kernel path, so 64 blocks at
         * any size and no streaming under any knob */
        {ZC_COLL_ALLREDUCE, false, 2, 4, 256 * M, 0, ZC_STREAM_AUTO, 64,
         false, false},
        {ZC_COLL_ALLREDUCE, false, 2, 4, 256 * M, 0, ZC_STREAM_ON, 64, false,
         false},
        {ZC_COLL_REDUCE_SCATTER, false, 4, 2, 160 * M, 0, ZC_STREAM_AUTO, 64,
         false, false},
        {ZC_COLL_OTHER, false, 8, 1, 256 * M, 96, ZC_STREAM_AUTO, 96, false,
         false},
        /* a negative override is no override */
        {ZC_COLL_ALLREDUCE, true, 2, 4, 256 * M, -1, ZC_STREAM_AUTO, 192,
         true},
        {ZC_COLL_ALLREDUCE, true, 2, 4, 4096, -5, ZC_STREAM_OFF, 64, false},
        {ZC_COLL_BCAST, true, 4, 2, 160 * M, -1, ZC_STREAM_ON, 128, false},
    };
    for (const Spot &s : spots) {
        const ZcPolicy p =
            zc_policy(s.ct, s.one, s.n, s.d, s.sz, s.single, s.ov, s.knob);
        cases++;
        if (p.blocks != s.blocks || p.stream != s.stream) {
            bad++;
            printf("SPOT ct=%d n=%d d=%d sz=%llu: blocks %d want %d, stream "
                   "%d want %d\n", (int)s.ct, s.n, s.d,
                   (unsigned long long)s.sz, p.blocks, s.blocks,
                   (int)p.stream, (int)s.stream);
        }
    }
    /* auto streams in exactly: allreduce, one-kernel, n 2, depth 4, the
     * four sizes from 128 MiB, four override values */
    if (streamed_auto != 4 * 4) {
        bad++;
        printf("auto streamed in %ld table cases, want 16\n", streamed_auto);
    }
    /* knob 1 streams in exactly: three collectives on k_zc_allreduce,
     * one-kernel, four rank counts, depth 4, seven sizes, four override
     * values */
    if (streamed_on != 3 * 4 * 7 * 4) {
        bad++;
        printf("knob 1 streamed in %ld table cases, want 336\n",
               streamed_on);
    }
    printf("cases=%ld bad=%ld\n", cases, bad);
    if (bad) {
        return 1;
    }
    printf("ZC_POLICY_OK\n");
    return 0;
}
