/* Host-only check of src/tl/cdna4/fused_plan.h: all ranks of a fused
 * allgather / reduce_scatter / alltoall / bcast / reduce simulated on host
 * memory, byte by byte: every rank stages its cells, then (the handshake)
 * every rank runs its copy segments and its reduce segment.
 *
 * Byte i of rank s's source vector is a value below 32, so that a byte-wise
 * sum over at most 8 ranks never carries: the reduction of count elements of
 * any element size is then the byte-wise sum, and the expected dst follows
 * from the collective's definition alone.
 *
 * Every user buffer keeps a write count per byte, every scratch a "staged"
 * mark per byte. Checked: the result; every scratch offset a multiple of
 * 16; every access inside its buffer resp. below scratch_bytes; every dst
 * byte the collective defines written exactly once and no other byte
 * written; only staged scratch read. Between the two phases an in-place
 * source is overwritten with garbage, so a result that is still right was
 * computed from staged data only. */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../src/tl/cdna4/fused_plan.h"

using namespace ucc;

static const char *kName[] = {"allgather", "reduce_scatter", "alltoall",
                              "bcast", "reduce"};
constexpr uint8_t kSentinel = 0xC3; /* dst fill before the collective */
constexpr uint8_t kGarbage  = 0xEE; /* in-place source after staging  */

static inline uint8_t val(int s, uint64_t i)
{
    return (uint8_t)(((uint64_t)s * 131 + i * 7 + (i >> 8)) & 0x1f);
}

struct Rank {
    FusedPlan            plan;
    std::vector<uint8_t> src, dst, dst_w;
    std::vector<uint8_t> scratch, staged;
};

struct Fail {
    const char *what = nullptr;
};

#define CHECK(cond, msg)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            f.what = msg;                                                    \
            return f;                                                        \
        }                                                                    \
    } while (0)

static Fail simulate(FusedColl coll, int n, int root, uint64_t b, size_t esz,
                     bool inplace)
{
    Fail              f;
    std::vector<Rank> rk((size_t)n);
    const uint64_t    nb = (uint64_t)n * b;
    /* ---- set-up: buffers by the collective's definition */
    for (int r = 0; r < n; r++) {
        Rank &k = rk[(size_t)r];
        CHECK(fused_plan_init(&k.plan, coll, n, r, root, b, esz, inplace),
              "plan refused");
        const FusedPlan &p = k.plan;
        CHECK(p.scratch_bytes == fused_plan_scratch_bytes(coll, n, b),
              "scratch_bytes differs from fused_plan_scratch_bytes");
        CHECK(p.scratch_bytes % 16 == 0, "scratch_bytes not 16-aligned");
        uint64_t src_sz = 0, dst_sz = 0;
        switch (coll) {
        case FUSED_ALLGATHER: src_sz = b; dst_sz = nb; break;
        case FUSED_REDUCE_SCATTER:
            src_sz = nb;
            dst_sz = inplace ? nb : b;
            break;
        case FUSED_ALLTOALL: src_sz = nb; dst_sz = nb; break;
        case FUSED_BCAST: src_sz = 0; dst_sz = b; break;
        case FUSED_REDUCE: src_sz = b; dst_sz = b; break;
        }
        k.dst.assign(dst_sz, kSentinel);
        k.dst_w.assign(dst_sz, 0);
        k.scratch.assign(p.scratch_bytes, 0x55);
        k.staged.assign(p.scratch_bytes, 0);
        /* where the source vector lives */
        bool want_sid = false;
        switch (coll) {
        case FUSED_ALLGATHER:
        case FUSED_REDUCE_SCATTER: want_sid = inplace; break;
        case FUSED_ALLTOALL: want_sid = false; break;
        case FUSED_BCAST: want_sid = true; break;
        case FUSED_REDUCE: want_sid = inplace && r == root; break;
        }
        CHECK(p.src_is_dst == want_sid, "src_is_dst wrong");
        if (p.src_is_dst) {
            if (coll == FUSED_ALLGATHER) {
                for (uint64_t i = 0; i < b; i++) {
                    k.dst[(uint64_t)r * b + i] = val(r, i);
                }
            } else if (coll != FUSED_BCAST || r == root) {
                for (uint64_t i = 0; i < dst_sz; i++) {
                    k.dst[i] = val(r, i);
                }
            }
        } else {
            k.src.resize(src_sz);
            for (uint64_t i = 0; i < src_sz; i++) {
                k.src[i] = val(r, i);
            }
        }
    }
    /* ---- phase 1: every rank stages */
    for (int r = 0; r < n; r++) {
        Rank            &k = rk[(size_t)r];
        const FusedPlan &p = k.plan;
        CHECK(p.n_cells >= 0 && p.n_cells <= kFusedMaxRanks, "n_cells");
        const std::vector<uint8_t> &from = p.src_is_dst ? k.dst : k.src;
        uint64_t                    sum  = 0;
        for (int c = 0; c < p.n_cells; c++) {
            const FusedCell &cl = p.cell[c];
            CHECK(cl.scratch_off % 16 == 0, "cell scratch_off not 16-aligned");
            CHECK(cl.scratch_off + cl.len <= p.scratch_bytes,
                  "cell beyond scratch_bytes");
            CHECK(cl.src_off + cl.len <= from.size(), "cell beyond source");
            for (uint64_t i = 0; i < cl.len; i++) {
                CHECK(!k.staged[cl.scratch_off + i], "scratch staged twice");
                k.scratch[cl.scratch_off + i] = from[cl.src_off + i];
                k.staged[cl.scratch_off + i]  = 1;
            }
            sum += cl.len;
        }
        CHECK(sum == p.stage_bytes, "stage_bytes");
        if (coll == FUSED_BCAST) {
            CHECK((p.n_cells != 0) == (r == root), "bcast: cells at non-root");
        }
    }
    /* ---- the handshake. From here on a source that aliases dst may be
     * overwritten at any time: make that the worst case. */
    for (int r = 0; r < n; r++) {
        Rank &k = rk[(size_t)r];
        if (k.plan.src_is_dst && coll != FUSED_BCAST) {
            for (auto &x : k.dst) {
                x = kGarbage;
            }
        }
    }
    /* ---- phase 2: every rank reads the peers' scratch */
    for (int r = 0; r < n; r++) {
        Rank            &k = rk[(size_t)r];
        const FusedPlan &p = k.plan;
        CHECK(p.n_segs >= 0 && p.n_segs <= kFusedMaxRanks, "n_segs");
        uint64_t rd = 0;
        for (int s = 0; s < p.n_segs; s++) {
            const FusedSeg &g = p.seg[s];
            CHECK(g.peer >= 0 && g.peer < n, "seg peer");
            CHECK(g.scratch_off % 16 == 0, "seg scratch_off not 16-aligned");
            CHECK(g.scratch_off + g.len <= p.scratch_bytes,
                  "seg beyond scratch_bytes");
            CHECK(g.dst_off + g.len <= k.dst.size(), "seg beyond dst");
            const Rank &pr = rk[(size_t)g.peer];
            for (uint64_t i = 0; i < g.len; i++) {
                CHECK(pr.staged[g.scratch_off + i], "seg reads unstaged");
                k.dst[g.dst_off + i] = pr.scratch[g.scratch_off + i];
                k.dst_w[g.dst_off + i]++;
            }
            rd += g.len;
        }
        if (p.red_count) {
            const uint64_t len = p.red_count * esz;
            CHECK(p.red_scratch_off % 16 == 0, "red scratch_off not aligned");
            CHECK(p.red_scratch_off + len <= p.scratch_bytes,
                  "reduce beyond scratch_bytes");
            CHECK(p.red_dst_off + len <= k.dst.size(), "reduce beyond dst");
            for (uint64_t i = 0; i < len; i++) {
                unsigned acc = 0;
                for (int s = 0; s < n; s++) {
                    CHECK(rk[(size_t)s].staged[p.red_scratch_off + i],
                          "reduce reads unstaged");
                    acc += rk[(size_t)s].scratch[p.red_scratch_off + i];
                }
                k.dst[p.red_dst_off + i] = (uint8_t)acc;
                k.dst_w[p.red_dst_off + i]++;
            }
            rd += len * (uint64_t)n;
        }
        CHECK(rd == p.read_bytes, "read_bytes");
        if (coll == FUSED_BCAST && r == root) {
            CHECK(p.n_segs == 0 && p.red_count == 0, "bcast root reads");
        }
        if (coll == FUSED_REDUCE && r != root) {
            CHECK(p.n_segs == 0 && p.red_count == 0, "reduce non-root reads");
        }
    }
    /* ---- the collective's definition */
    for (int r = 0; r < n; r++) {
        const Rank &k = rk[(size_t)r];
        for (uint64_t i = 0; i < k.dst.size(); i++) {
            bool     defined = false;
            unsigned exp     = 0;
            switch (coll) {
            case FUSED_ALLGATHER:
                defined = true;
                exp     = val((int)(i / b), i % b);
                break;
            case FUSED_ALLTOALL:
                defined = true;
                exp     = val((int)(i / b), (uint64_t)r * b + i % b);
                break;
            case FUSED_REDUCE_SCATTER: {
                const uint64_t lo = inplace ? (uint64_t)r * b : 0;
                defined           = i >= lo && i < lo + b;
                for (int s = 0; defined && s < n; s++) {
                    exp += val(s, (uint64_t)r * b + (i - lo));
                }
                break;
            }
            case FUSED_BCAST:
                defined = r != root;
                exp     = val(root, i);
                break;
            case FUSED_REDUCE:
                defined = r == root;
                for (int s = 0; defined && s < n; s++) {
                    exp += val(s, i);
                }
                break;
            }
            if (defined) {
                CHECK(k.dst_w[i] == 1, "defined dst byte not written once");
                CHECK(k.dst[i] == (uint8_t)exp, "wrong result");
            } else {
                CHECK(k.dst_w[i] == 0, "undefined dst byte written");
            }
        }
        if (coll == FUSED_REDUCE && r != root) {
            for (auto x : k.dst) {
                CHECK(x == kSentinel, "reduce touched a non-root dst");
            }
        }
        if (coll == FUSED_BCAST && r == root) {
            for (uint64_t i = 0; i < b; i++) {
                CHECK(k.dst[i] == val(root, i), "bcast changed the root");
            }
        }
    }
    return f;
}

int main()
{
    const uint64_t counts[] = {1, 7, 999, 4097};
    const size_t   eszs[]   = {1, 2, 4, 8, 16};
    uint64_t       sims     = 0;
    for (int n = 2; n <= kFusedMaxRanks; n++) {
        for (int ci = 0; ci < 5; ci++) {
            const FusedColl coll = (FusedColl)ci;
            const bool rooted = coll == FUSED_BCAST || coll == FUSED_REDUCE;
            for (int root = 0; root < (rooted ? n : 1); root++) {
                for (uint64_t cnt : counts) {
                    for (size_t esz : eszs) {
                        for (int ip = 0; ip < 2; ip++) {
                            if (ip && coll == FUSED_ALLTOALL) {
                                continue; /* declined, checked below */
                            }
                            Fail f = simulate(coll, n, root, cnt * esz, esz,
                                              ip != 0);
                            if (f.what) {
                                printf("FAIL %s n=%d root=%d count=%llu "
                                       "esz=%zu inplace=%d: %s\n",
                                       kName[ci], n, root,
                                       (unsigned long long)cnt, esz, ip,
                                       f.what);
                                return 1;
                            }
                            sims++;
                        }
                    }
                }
            }
        }
    }
    /* what the plan must refuse */
    FusedPlan p;
    const bool refused =
        !fused_plan_init(&p, FUSED_ALLTOALL, 4, 0, 0, 64, 4, true) &&
        !fused_plan_init(&p, FUSED_ALLGATHER, 1, 0, 0, 64, 4, false) &&
        !fused_plan_init(&p, FUSED_ALLGATHER, kFusedMaxRanks + 1, 0, 0, 64, 4,
                         false) &&
        !fused_plan_init(&p, FUSED_BCAST, 4, 4, 0, 64, 4, false) &&
        !fused_plan_init(&p, FUSED_BCAST, 4, 0, 4, 64, 4, false) &&
        !fused_plan_init(&p, FUSED_REDUCE, 4, 0, 0, 0, 4, false) &&
        !fused_plan_init(&p, FUSED_REDUCE, 4, 0, 0, 66, 4, false);
    if (!refused) {
        printf("FAIL an inexpressible plan was accepted\n");
        return 1;
    }
    /* the bound is on a rank-invariant number: 16-byte cells */
    if (fused_plan_scratch_bytes(FUSED_ALLGATHER, 8, 1998) != 2000 ||
        fused_plan_scratch_bytes(FUSED_ALLTOALL, 8, 1998) != 16000 ||
        fused_plan_scratch_bytes(FUSED_REDUCE, 8, 1) != 16) {
        printf("FAIL scratch_bytes\n");
        return 1;
    }
    printf("FUSED_PLAN_OK sims=%llu\n", (unsigned long long)sims);
    return 0;
}
