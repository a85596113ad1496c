/* Host-only check of the v-forms of src/tl/cdna4/fused_plan.h
 * (fused_plan_init_v): all ranks of a fused allgatherv / reduce_scatterv /
 * alltoallv simulated on host memory, byte by byte, in the kernel's order:
 * every rank stages its cells, (the handshake,) for alltoallv the verdict is
 * taken from all votes, then every rank runs its copy segments and its
 * reduce segment.
 *
 * Data bytes are below 32, so a byte-wise sum over at most 8 ranks never
 * carries and the reduction of any element size is the byte-wise sum.
 *
 * Every user buffer lies between two guard bands and keeps a write count
 * per byte. Checked: the collective's definition; every defined dst byte
 * written exactly once, no other byte (gaps between displaced blocks, the
 * bands) written; every scratch offset a multiple of 16 and every access
 * below scratch_bytes; only staged scratch read; scratch_bytes and the
 * alltoallv cell equal on all ranks. An in-place source is overwritten with
 * garbage between the phases. For alltoallv: one pair of exactly `cell`
 * bytes fits; one pair of cell + one element makes the verdict "does not
 * fit" on every rank, also on ranks whose own row and column fit, and then
 * nothing is read and no dst byte written. */
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../src/tl/cdna4/fused_plan.h"

using namespace ucc;

constexpr uint8_t  kSentinel = 0xC3;
constexpr uint8_t  kGarbage  = 0xEE;
constexpr uint64_t kBand     = 48; /* guard bytes on each side */
constexpr uint64_t kCell     = 16384;

static inline uint8_t val(int s, uint64_t i)
{
    return (uint8_t)(((uint64_t)s * 131 + i * 7 + (i >> 8)) & 0x1f);
}

struct Rng {
    uint64_t s;
    uint32_t next()
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
    uint32_t below(uint32_t n) { return next() % n; }
};

/* a user buffer: `size` bytes at kBand inside a sentinel-filled vector */
struct Buf {
    std::vector<uint8_t> b, w;
    uint64_t             size = 0;
    void init(uint64_t n)
    {
        size = n;
        b.assign(n + 2 * kBand, kSentinel);
        w.assign(n + 2 * kBand, 0);
    }
    uint8_t &at(uint64_t i) { return b[kBand + i]; }
    void     put(uint64_t i, uint8_t v)
    {
        b[kBand + i] = v;
        w[kBand + i]++;
    }
};

struct Rank {
    FusedPlan             plan;
    Buf                   src, dst;
    std::vector<uint8_t>  scratch, staged;
    std::vector<uint8_t>  defined, expect; /* over dst.b */
    std::vector<uint64_t> sc, sd, rc, rd;  /* bytes */
};

static const char *g_what = nullptr;
#define CHECK(cond, msg)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            g_what = msg;                                                    \
            return false;                                                    \
        }                                                                    \
    } while (0)

/* element counts of the blocks: zeros, 1 and 7 (lengths that are no
 * multiple of 16), 999, and small random ones */
static uint64_t pick_count(Rng &g)
{
    switch (g.below(6)) {
    case 0: return 0;
    case 1: return 1;
    case 2: return 7;
    case 3: return 999;
    default: return 1 + g.below(300);
    }
}

/* displacements of n blocks, permuted and with gaps; returns the extent */
static uint64_t layout(Rng &g, int n, const std::vector<uint64_t> &cnt,
                       std::vector<uint64_t> *dsp, size_t esz)
{
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; i++) {
        order[(size_t)i] = i;
    }
    for (int i = n - 1; i > 0; i--) {
        std::swap(order[(size_t)i], order[g.below((uint32_t)i + 1)]);
    }
    uint64_t off = 0;
    dsp->assign((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        off += g.below(4) * esz; /* gap, in whole elements */
        (*dsp)[(size_t)order[(size_t)i]] = off;
        off += cnt[(size_t)order[(size_t)i]];
    }
    return off + g.below(4) * esz;
}

/* phases 1 and 2 for all ranks, then the comparison with `expect` */
static bool run(std::vector<Rank> &rk, FusedColl coll, int n, size_t esz,
                bool *verdict_out)
{
    uint64_t sb = rk[0].plan.scratch_bytes, cell = rk[0].plan.cell_bytes;
    for (int r = 0; r < n; r++) {
        Rank            &k = rk[(size_t)r];
        const FusedPlan &p = k.plan;
        CHECK(p.scratch_bytes == sb, "scratch_bytes differs between ranks");
        CHECK(p.cell_bytes == cell, "cell differs between ranks");
        CHECK(sb % 16 == 0, "scratch_bytes not 16-aligned");
        k.scratch.assign(sb, 0x55);
        k.staged.assign(sb, 0);
        CHECK(p.n_cells >= 0 && p.n_cells <= kFusedMaxRanks, "n_cells");
        Buf     &from = p.src_is_dst ? k.dst : k.src;
        uint64_t sum  = 0;
        if (coll == FUSED_ALLTOALLV) {
            CHECK(p.fits_local || p.n_cells == 0, "unfit rank stages");
        }
        for (int c = 0; c < p.n_cells; c++) {
            const FusedCell &cl = p.cell[c];
            CHECK(cl.len > 0, "empty cell");
            CHECK(cl.scratch_off % 16 == 0, "cell scratch_off not aligned");
            CHECK(coll != FUSED_ALLTOALLV || cl.scratch_off >= 16,
                  "cell on the header");
            CHECK(cl.scratch_off + cl.len <= sb, "cell beyond scratch_bytes");
            CHECK(cl.src_off + cl.len <= from.size, "cell beyond source");
            for (uint64_t i = 0; i < cl.len; i++) {
                CHECK(!k.staged[cl.scratch_off + i], "scratch staged twice");
                k.scratch[cl.scratch_off + i] = from.at(cl.src_off + i);
                k.staged[cl.scratch_off + i]  = 1;
            }
            sum += cl.len;
        }
        CHECK(sum == p.stage_bytes, "stage_bytes");
    }
    /* the handshake: an in-place source may now be overwritten */
    for (int r = 0; r < n; r++) {
        Rank &k = rk[(size_t)r];
        if (k.plan.src_is_dst) {
            for (uint64_t i = 0; i < k.dst.size; i++) {
                k.dst.at(i) = kGarbage;
            }
        }
    }
    bool votes[kFusedMaxRanks];
    for (int r = 0; r < n; r++) {
        votes[r] = rk[(size_t)r].plan.fits_local;
    }
    const bool fits =
        coll != FUSED_ALLTOALLV || fused_plan_a2av_verdict(votes, n);
    *verdict_out = fits;
    for (int r = 0; r < n; r++) {
        Rank            &k = rk[(size_t)r];
        const FusedPlan &p = k.plan;
        CHECK(p.n_segs >= 0 && p.n_segs <= kFusedMaxRanks, "n_segs");
        uint64_t rdb = 0;
        for (int s = 0; fits && s < p.n_segs; s++) {
            const FusedSeg &g = p.seg[s];
            CHECK(g.len > 0, "empty segment");
            CHECK(g.peer >= 0 && g.peer < n, "seg peer");
            CHECK(g.scratch_off % 16 == 0, "seg scratch_off not aligned");
            CHECK(g.scratch_off + g.len <= sb, "seg beyond scratch_bytes");
            CHECK(g.dst_off + g.len <= k.dst.size, "seg beyond dst");
            const Rank &pr = rk[(size_t)g.peer];
            for (uint64_t i = 0; i < g.len; i++) {
                CHECK(pr.staged[g.scratch_off + i], "seg reads unstaged");
                k.dst.put(g.dst_off + i, pr.scratch[g.scratch_off + i]);
            }
            rdb += g.len;
        }
        if (p.red_count) {
            const uint64_t len = p.red_count * esz;
            CHECK(p.red_scratch_off % 16 == 0, "red scratch_off not aligned");
            CHECK(p.red_scratch_off + len <= sb, "reduce beyond scratch");
            CHECK(p.red_dst_off + len <= k.dst.size, "reduce beyond dst");
            for (uint64_t i = 0; i < len; i++) {
                unsigned acc = 0;
                for (int s = 0; s < n; s++) {
                    CHECK(rk[(size_t)s].staged[p.red_scratch_off + i],
                          "reduce reads unstaged");
                    acc += rk[(size_t)s].scratch[p.red_scratch_off + i];
                }
                k.dst.put(p.red_dst_off + i, (uint8_t)acc);
            }
            rdb += len * (uint64_t)n;
        }
        CHECK(!fits || rdb == p.read_bytes, "read_bytes");
    }
    for (int r = 0; r < n; r++) {
        Rank &k = rk[(size_t)r];
        for (uint64_t i = 0; i < k.dst.b.size(); i++) {
            if (fits && k.defined[i]) {
                CHECK(k.dst.w[i] == 1, "defined dst byte not written once");
                CHECK(k.dst.b[i] == k.expect[i], "wrong result");
            } else {
                CHECK(k.dst.w[i] == 0, "undefined dst byte written");
                CHECK(k.plan.src_is_dst || k.dst.b[i] == kSentinel,
                      "canary changed");
            }
        }
        /* the bands, whatever the garbage pass did inside */
        for (uint64_t i = 0; i < kBand; i++) {
            CHECK(k.dst.b[i] == kSentinel &&
                      k.dst.b[kBand + k.dst.size + i] == kSentinel,
                  "dst band changed");
        }
    }
    return true;
}

static bool sim_agv(Rng &g, int n, size_t esz, bool inplace)
{
    std::vector<uint64_t> cnt((size_t)n), dsp;
    for (auto &c : cnt) {
        c = pick_count(g) * esz;
    }
    cnt[g.below((uint32_t)n)] = 0;
    cnt[g.below((uint32_t)n)] = 7 * esz; /* at least one non-zero */
    const uint64_t ext = layout(g, n, cnt, &dsp, esz);
    std::vector<Rank> rk((size_t)n);
    for (int r = 0; r < n; r++) {
        Rank &k = rk[(size_t)r];
        CHECK(fused_plan_init_v(&k.plan, FUSED_ALLGATHERV, n, r, cnt.data(),
                                dsp.data(), nullptr, nullptr, 0, esz,
                                inplace),
              "plan refused");
        CHECK(k.plan.src_is_dst == inplace, "src_is_dst");
        uint64_t mx = 0;
        for (auto c : cnt) {
            mx = std::max(mx, fused_plan_stride(c));
        }
        CHECK(k.plan.scratch_bytes == mx, "scratch_bytes != stride(max)");
        k.dst.init(ext);
        k.src.init(inplace ? 0 : cnt[(size_t)r]);
        for (uint64_t i = 0; i < cnt[(size_t)r]; i++) {
            (inplace ? k.dst.at(dsp[(size_t)r] + i) : k.src.at(i)) =
                val(r, i);
        }
        k.defined.assign(k.dst.b.size(), 0);
        k.expect.assign(k.dst.b.size(), 0);
        for (int s = 0; s < n; s++) {
            for (uint64_t i = 0; i < cnt[(size_t)s]; i++) {
                k.defined[kBand + dsp[(size_t)s] + i] = 1;
                k.expect[kBand + dsp[(size_t)s] + i]  = val(s, i);
            }
        }
    }
    bool fits;
    return run(rk, FUSED_ALLGATHERV, n, esz, &fits);
}

static bool sim_rsv(Rng &g, int n, size_t esz, bool inplace)
{
    std::vector<uint64_t> cnt((size_t)n), off((size_t)n);
    for (auto &c : cnt) {
        c = pick_count(g) * esz;
    }
    cnt[g.below((uint32_t)n)] = 1 * esz;
    const int zero = (int)g.below((uint32_t)n);
    cnt[(size_t)zero]  = 0; /* stages and shakes hands, no reduce segment */
    cnt[(size_t)((zero + 1) % n)] += 7 * esz;
    uint64_t total = 0, strides = 0;
    for (int r = 0; r < n; r++) {
        off[(size_t)r] = total;
        total += cnt[(size_t)r];
        strides += fused_plan_stride(cnt[(size_t)r]);
    }
    /* displacements are ignored: pass nonsense */
    std::vector<uint64_t> junk((size_t)n, 0xdeadbeef);
    std::vector<Rank>     rk((size_t)n);
    for (int r = 0; r < n; r++) {
        Rank &k = rk[(size_t)r];
        CHECK(fused_plan_init_v(&k.plan, FUSED_REDUCE_SCATTERV, n, r,
                                cnt.data(), junk.data(), nullptr, nullptr, 0,
                                esz, inplace),
              "plan refused");
        CHECK(k.plan.scratch_bytes == strides, "scratch_bytes != strides");
        CHECK((k.plan.red_count == 0) == (cnt[(size_t)r] == 0),
              "reduce segment of a zero count");
        CHECK(k.plan.stage_bytes == total, "a rank must stage every cell");
        k.dst.init(inplace ? total : cnt[(size_t)r]);
        k.src.init(inplace ? 0 : total);
        for (uint64_t i = 0; i < total; i++) {
            (inplace ? k.dst.at(i) : k.src.at(i)) = val(r, i);
        }
        k.defined.assign(k.dst.b.size(), 0);
        k.expect.assign(k.dst.b.size(), 0);
        const uint64_t lo = inplace ? off[(size_t)r] : 0;
        for (uint64_t i = 0; i < cnt[(size_t)r]; i++) {
            unsigned e = 0;
            for (int s = 0; s < n; s++) {
                e += val(s, off[(size_t)r] + i);
            }
            k.defined[kBand + lo + i] = 1;
            k.expect[kBand + lo + i]  = (uint8_t)e;
        }
    }
    bool fits;
    return run(rk, FUSED_REDUCE_SCATTERV, n, esz, &fits);
}

/* special: 0 = random matrix, 1 = one pair of exactly cell bytes, 2 = one
 * pair of cell + one element */
static bool sim_a2av(Rng &g, int n, size_t esz, int special)
{
    const uint64_t cell = fused_plan_a2av_cell(16 + (uint64_t)n * kCell, n);
    CHECK(cell == kCell, "cell");
    /* m[s][d]: bytes rank s sends to rank d */
    std::vector<std::vector<uint64_t>> m(
        (size_t)n, std::vector<uint64_t>((size_t)n, 0));
    for (auto &row : m) {
        for (auto &c : row) {
            c = pick_count(g) * esz;
        }
    }
    const int zs = (int)g.below((uint32_t)n); /* sends nothing    */
    const int zr = (int)g.below((uint32_t)n); /* receives nothing */
    for (int i = 0; i < n; i++) {
        m[(size_t)zs][(size_t)i] = 0;
        m[(size_t)i][(size_t)zr] = 0;
    }
    int a = (zs + 1) % n, b = (zr + 1) % n; /* a sends, b receives */
    m[(size_t)a][(size_t)b] = 7 * esz;
    if (special) {
        m[(size_t)a][(size_t)b] = cell + (special == 2 ? esz : 0);
    }
    std::vector<Rank> rk((size_t)n);
    int               fit_ranks = 0;
    for (int r = 0; r < n; r++) {
        Rank &k = rk[(size_t)r];
        k.sc    = m[(size_t)r];
        k.rc.assign((size_t)n, 0);
        for (int s = 0; s < n; s++) {
            k.rc[(size_t)s] = m[(size_t)s][(size_t)r];
        }
        const uint64_t sext = layout(g, n, k.sc, &k.sd, esz);
        const uint64_t rext = layout(g, n, k.rc, &k.rd, esz);
        CHECK(fused_plan_init_v(&k.plan, FUSED_ALLTOALLV, n, r, k.sc.data(),
                                k.sd.data(), k.rc.data(), k.rd.data(), cell,
                                1, false),
              "plan refused");
        CHECK(k.plan.scratch_bytes == 16 + (uint64_t)n * cell,
              "scratch_bytes != header + n cells");
        CHECK(!k.plan.src_is_dst, "src_is_dst");
        const bool row_fits =
            *std::max_element(k.sc.begin(), k.sc.end()) <= cell;
        CHECK(k.plan.fits_local == row_fits, "fits_local");
        fit_ranks += k.plan.fits_local;
        k.src.init(sext);
        k.dst.init(rext);
        for (int d = 0; d < n; d++) {
            for (uint64_t i = 0; i < k.sc[(size_t)d]; i++) {
                k.src.at(k.sd[(size_t)d] + i) = val(r * 8 + d, i);
            }
        }
        k.defined.assign(k.dst.b.size(), 0);
        k.expect.assign(k.dst.b.size(), 0);
        for (int s = 0; s < n; s++) {
            for (uint64_t i = 0; i < k.rc[(size_t)s]; i++) {
                k.defined[kBand + k.rd[(size_t)s] + i] = 1;
                k.expect[kBand + k.rd[(size_t)s] + i]  = val(s * 8 + r, i);
            }
        }
    }
    bool fits = false;
    if (!run(rk, FUSED_ALLTOALLV, n, esz, &fits)) {
        return false;
    }
    CHECK(fits == (special != 2), "verdict");
    if (special == 2) {
        /* only the sender of the oversized pair votes no; every other
         * rank's row fits (and for n > 2 some rank's column too), yet run()
         * saw no dst byte written anywhere */
        CHECK(fit_ranks == n - 1, "exactly one rank must vote no");
    }
    return true;
}

int main()
{
    const size_t eszs[] = {1, 2, 4, 8, 16};
    uint64_t     sims   = 0;
    for (int n = 2; n <= kFusedMaxRanks; n++) {
        for (size_t esz : eszs) {
            for (uint64_t seed = 1; seed <= 6; seed++) {
                Rng g{seed * 1000003 + (uint64_t)n * 101 + esz};
                for (int variant = 0; variant < 7; variant++) {
                    bool        ok   = false;
                    const char *name = "";
                    switch (variant) {
                    case 0:
                    case 1:
                        name = "allgatherv";
                        ok   = sim_agv(g, n, esz, variant == 1);
                        break;
                    case 2:
                    case 3:
                        name = "reduce_scatterv";
                        ok   = sim_rsv(g, n, esz, variant == 3);
                        break;
                    default:
                        name = "alltoallv";
                        ok   = sim_a2av(g, n, esz, variant - 4);
                        break;
                    }
                    if (!ok) {
                        printf("FAIL %s n=%d esz=%zu seed=%llu variant=%d: "
                               "%s\n",
                               name, n, esz, (unsigned long long)seed,
                               variant, g_what);
                        return 1;
                    }
                    sims++;
                }
            }
        }
    }
    /* what the plan must refuse */
    FusedPlan      p;
    const uint64_t c4[4] = {64, 0, 6, 64}, z4[4] = {0, 0, 0, 0},
                   d4[4] = {0, 64, 64, 80};
    const bool refused =
        !fused_plan_init_v(&p, FUSED_ALLTOALLV, 4, 0, c4, d4, c4, d4, 64, 1,
                           true) &&
        !fused_plan_init_v(&p, FUSED_ALLTOALLV, 4, 0, c4, d4, c4, d4, 0, 1,
                           false) &&
        !fused_plan_init_v(&p, FUSED_ALLTOALLV, 4, 0, c4, d4, c4, d4, 24, 1,
                           false) &&
        !fused_plan_init_v(&p, FUSED_ALLGATHERV, 4, 0, z4, d4, nullptr,
                           nullptr, 0, 2, false) &&
        !fused_plan_init_v(&p, FUSED_REDUCE_SCATTERV, 4, 0, z4, d4, nullptr,
                           nullptr, 0, 2, false) &&
        !fused_plan_init_v(&p, FUSED_REDUCE_SCATTERV, 4, 0, c4, d4, nullptr,
                           nullptr, 0, 4, false) &&
        !fused_plan_init_v(&p, FUSED_ALLGATHERV, 1, 0, c4, d4, nullptr,
                           nullptr, 0, 2, false) &&
        !fused_plan_init_v(&p, FUSED_ALLGATHERV, kFusedMaxRanks + 1, 0, c4,
                           d4, nullptr, nullptr, 0, 2, false) &&
        !fused_plan_init_v(&p, FUSED_ALLGATHER, 4, 0, c4, d4, nullptr,
                           nullptr, 0, 2, false);
    if (!refused) {
        printf("FAIL an inexpressible v-plan was accepted\n");
        return 1;
    }
    /* the bounds are on rank-invariant numbers */
    if (fused_plan_a2av_cell(8192, 8) != 1008 ||
        fused_plan_a2av_cell(16 + 2 * 16, 2) != 16 ||
        fused_plan_a2av_cell(16 + 2 * 16 - 1, 2) != 0 ||
        fused_plan_a2av_cell(15, 2) != 0 ||
        fused_plan_scratch_bytes_v(FUSED_ALLGATHERV, 4, c4, 0) != 64 ||
        fused_plan_scratch_bytes_v(FUSED_REDUCE_SCATTERV, 4, c4, 0) != 144 ||
        fused_plan_scratch_bytes_v(FUSED_ALLTOALLV, 4, nullptr, 1008) !=
            16 + 4 * 1008) {
        printf("FAIL v scratch_bytes\n");
        return 1;
    }
    printf("FUSED_PLAN_V_OK sims=%llu\n", (unsigned long long)sims);
    return 0;
}
