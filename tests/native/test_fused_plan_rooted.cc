/* Host-only check of the rooted copy collectives of
 * src/tl/cdna4/fused_plan.h: gather and scatter (fused_plan_init) and gatherv
 * and scatterv (fused_plan_init_rooted_v, fused_plan_rooted_v_verdict). All
 * ranks are simulated on host memory, byte by byte, in the kernel's order:
 * every rank stages its cells, (the handshake,) for the v-forms the root's
 * verdict and table are read, then every rank runs its copy segments; a
 * non-root of scatterv takes its one segment from the root's table, as
 * k_fused_rooted_v does.
 *
 * Every user buffer lies between two guard bands and keeps a write count per
 * byte. Checked: the collective's definition; every defined dst byte written
 * exactly once; gaps between displaced blocks, the bands, the root's own
 * block when in place and every non-root dst of gather(v) never written;
 * every scratch offset a multiple of 16 and every access below
 * scratch_bytes; only staged scratch read; scratch_bytes and the bound B
 * equal on all ranks. For the v-forms: a count of exactly B fits, B plus one
 * element does not, at the root's own index and at another rank's; for
 * scatterv a stride sum of exactly B fits and B + 16 does not; a "does not
 * fit" verdict reads and writes nothing after the handshake; a rank whose
 * own length disagrees with the root's table copies the smaller of the two
 * and stays inside its dst. */
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../src/tl/cdna4/fused_plan.h"

using namespace ucc;

constexpr uint8_t  kSentinel = 0xC3;
constexpr uint64_t kBand     = 48; /* guard bytes on each side */

static inline uint8_t val(int s, uint64_t i)
{
    return (uint8_t)(((uint64_t)s * 131 + i * 7 + (i >> 8)) & 0x7f);
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

/* what a dst byte must be afterwards */
enum : uint8_t {
    kUntouched = 0, /* never written, still the sentinel                   */
    kWritten   = 1, /* written exactly once, == expect                     */
    kKept      = 2  /* never written, still == expect (in place, at root)  */
};

struct Rank {
    FusedPlan            plan;
    Buf                  src, dst;
    std::vector<uint8_t> scratch, staged;
    std::vector<uint8_t> state, expect; /* over dst.b */
    void                 expect_init()
    {
        state.assign(dst.b.size(), kUntouched);
        expect.assign(dst.b.size(), 0);
    }
    void want(uint64_t i, uint8_t v, uint8_t st = kWritten)
    {
        state[kBand + i]  = st;
        expect[kBand + i] = v;
    }
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

/* one copy segment of rank k, with every check an access needs */
static bool copy_seg(std::vector<Rank> &rk, Rank &k, int n, int peer,
                     uint64_t sc_off, uint64_t dst_off, uint64_t len,
                     uint64_t sb)
{
    CHECK(len > 0, "empty segment");
    CHECK(peer >= 0 && peer < n, "seg peer");
    CHECK(sc_off % 16 == 0, "seg scratch_off not aligned");
    CHECK(sc_off + len <= sb, "seg beyond scratch_bytes");
    CHECK(dst_off + len <= k.dst.size, "seg beyond dst");
    const Rank &pr = rk[(size_t)peer];
    for (uint64_t i = 0; i < len; i++) {
        CHECK(pr.staged[sc_off + i], "seg reads unstaged");
        k.dst.put(dst_off + i, pr.scratch[sc_off + i]);
    }
    return true;
}

/* Both phases for all ranks, then the comparison with `expect`. rooted_v:
 * the plans are fused_plan_init_rooted_v's, and what runs after the
 * handshake is decided by fused_plan_rooted_v_verdict from the root's plan;
 * `fits_out` gets that verdict. */
static bool run(std::vector<Rank> &rk, int n, int root, bool rooted_v,
                bool *fits_out)
{
    const uint64_t sb = rk[0].plan.scratch_bytes, B = rk[0].plan.bound;
    const uint64_t lo = rooted_v ? kFusedRootedHdr : 0;
    CHECK(sb % 16 == 0, "scratch_bytes not 16-aligned");
    for (int r = 0; r < n; r++) {
        Rank            &k = rk[(size_t)r];
        const FusedPlan &p = k.plan;
        CHECK(p.scratch_bytes == sb, "scratch_bytes differs between ranks");
        CHECK(p.bound == B, "B differs between ranks");
        CHECK(!rooted_v || sb == kFusedRootedHdr + B, "scratch_bytes != 144+B");
        CHECK(!p.src_is_dst && p.red_count == 0, "not a rooted copy plan");
        k.scratch.assign(sb, 0x55);
        k.staged.assign(sb, 0);
        CHECK(p.n_cells >= 0 && p.n_cells <= kFusedMaxRanks, "n_cells");
        CHECK(!rooted_v || p.fits_local || p.n_cells == 0,
              "a rank that does not fit stages");
        uint64_t sum = 0;
        for (int c = 0; c < p.n_cells; c++) {
            const FusedCell &cl = p.cell[c];
            CHECK(cl.len > 0, "empty cell");
            CHECK(cl.scratch_off % 16 == 0, "cell scratch_off not aligned");
            CHECK(cl.scratch_off >= lo, "cell on the header");
            CHECK(cl.scratch_off + cl.len <= sb, "cell beyond scratch_bytes");
            CHECK(cl.src_off + cl.len <= k.src.size, "cell beyond source");
            for (uint64_t i = 0; i < cl.len; i++) {
                CHECK(!k.staged[cl.scratch_off + i], "scratch staged twice");
                k.scratch[cl.scratch_off + i] = k.src.at(cl.src_off + i);
                k.staged[cl.scratch_off + i]  = 1;
            }
            sum += cl.len;
        }
        CHECK(sum == p.stage_bytes, "stage_bytes");
    }
    /* the handshake */
    const FusedPlan &rp   = rk[(size_t)root].plan;
    bool             fits = true;
    for (int r = 0; r < n; r++) {
        Rank            &k = rk[(size_t)r];
        const FusedPlan &p = k.plan;
        CHECK(p.n_segs >= 0 && p.n_segs <= kFusedMaxRanks, "n_segs");
        uint64_t off = 0, len = 0;
        if (rooted_v) {
            const bool f =
                fused_plan_rooted_v_verdict(rp, r, p.my_len, &off, &len);
            CHECK(r == 0 || f == fits, "verdict differs between ranks");
            fits = f;
            CHECK(f == rp.fits_local, "verdict is not the root's");
        }
        if (!fits) {
            continue; /* nothing is read, nothing written */
        }
        if (rooted_v && p.coll == FUSED_SCATTERV && r != root) {
            /* the plan knows the dst length only */
            CHECK(p.n_segs == (p.my_len ? 1 : 0), "scatterv non-root segs");
            CHECK(p.n_segs == 0 || (p.seg[0].len == p.my_len &&
                                    p.seg[0].dst_off == 0 &&
                                    p.seg[0].peer == root),
                  "scatterv non-root segment");
            CHECK(len <= p.my_len, "table length beyond my dst");
            if (len && !copy_seg(rk, k, n, root, off, 0, len, sb)) {
                return false;
            }
            continue;
        }
        CHECK(r == root || p.n_segs == 0 || p.coll == FUSED_SCATTER,
              "a non-root reads");
        uint64_t rdb = 0;
        for (int s = 0; s < p.n_segs; s++) {
            const FusedSeg &g = p.seg[s];
            CHECK(g.scratch_off >= lo, "seg on the header");
            if (!copy_seg(rk, k, n, g.peer, g.scratch_off, g.dst_off, g.len,
                          sb)) {
                return false;
            }
            rdb += g.len;
        }
        CHECK(rdb == p.read_bytes, "read_bytes");
    }
    *fits_out = fits;
    for (int r = 0; r < n; r++) {
        Rank &k = rk[(size_t)r];
        for (uint64_t i = 0; i < k.dst.b.size(); i++) {
            const uint8_t st = k.state[i];
            if (st == kWritten && fits) {
                CHECK(k.dst.w[i] == 1, "defined dst byte not written once");
                CHECK(k.dst.b[i] == k.expect[i], "wrong result");
            } else if (st == kKept) {
                CHECK(k.dst.w[i] == 0, "in-place block written");
                CHECK(k.dst.b[i] == k.expect[i], "in-place block changed");
            } else {
                CHECK(k.dst.w[i] == 0, "undefined dst byte written");
                CHECK(k.dst.b[i] == kSentinel, "canary changed");
            }
        }
    }
    return true;
}

/* ------------------------------------------------------ gather, scatter */
static bool sim_gather(int n, int root, size_t esz, uint64_t elems, bool ip)
{
    const uint64_t    b = elems * esz;
    std::vector<Rank> rk((size_t)n);
    for (int r = 0; r < n; r++) {
        Rank      &k     = rk[(size_t)r];
        const bool mine_ip = ip && r == root;
        /* the flag is significant at the root only: a non-root passes it
         * too and must get the same plan */
        CHECK(fused_plan_init(&k.plan, FUSED_GATHER, n, r, root, b, esz, ip),
              "plan refused");
        CHECK(k.plan.scratch_bytes == fused_plan_stride(b) &&
                  k.plan.scratch_bytes ==
                      fused_plan_scratch_bytes(FUSED_GATHER, n, b),
              "scratch_bytes != stride(b)");
        CHECK(k.plan.n_cells == (mine_ip ? 0 : 1), "gather cells");
        CHECK(k.plan.n_segs == (r != root ? 0 : ip ? n - 1 : n),
              "gather segments");
        k.src.init(mine_ip ? 0 : b);
        k.dst.init(r == root ? (uint64_t)n * b : 32);
        k.expect_init();
        for (uint64_t i = 0; !mine_ip && i < b; i++) {
            k.src.at(i) = val(r, i);
        }
        for (int s = 0; r == root && s < n; s++) {
            for (uint64_t i = 0; i < b; i++) {
                const bool kept = ip && s == root;
                if (kept) {
                    k.dst.at((uint64_t)s * b + i) = val(s, i);
                }
                k.want((uint64_t)s * b + i, val(s, i),
                       kept ? kKept : kWritten);
            }
        }
    }
    bool fits;
    return run(rk, n, root, false, &fits);
}

static bool sim_scatter(int n, int root, size_t esz, uint64_t elems, bool ip)
{
    const uint64_t    b = elems * esz;
    std::vector<Rank> rk((size_t)n);
    for (int r = 0; r < n; r++) {
        Rank      &k       = rk[(size_t)r];
        const bool mine_ip = ip && r == root;
        CHECK(fused_plan_init(&k.plan, FUSED_SCATTER, n, r, root, b, esz, ip),
              "plan refused");
        CHECK(k.plan.scratch_bytes == (uint64_t)n * fused_plan_stride(b) &&
                  k.plan.scratch_bytes ==
                      fused_plan_scratch_bytes(FUSED_SCATTER, n, b),
              "scratch_bytes != n * stride(b)");
        CHECK(k.plan.n_cells == (r != root ? 0 : ip ? n - 1 : n),
              "scatter cells");
        CHECK(k.plan.n_segs == (mine_ip ? 0 : 1), "scatter segments");
        k.src.init(r == root ? (uint64_t)n * b : 0);
        k.dst.init(mine_ip ? 0 : b);
        k.expect_init();
        for (int d = 0; r == root && d < n; d++) {
            for (uint64_t i = 0; i < b; i++) {
                k.src.at((uint64_t)d * b + i) = val(d, i);
            }
        }
        for (uint64_t i = 0; !mine_ip && i < b; i++) {
            k.want(i, val(r, i));
        }
    }
    std::vector<uint8_t> src_before = rk[(size_t)root].src.b;
    bool                 fits;
    if (!run(rk, n, root, false, &fits)) {
        return false;
    }
    CHECK(rk[(size_t)root].src.b == src_before, "the root's src changed");
    return true;
}

/* ---------------------------------------------------- gatherv, scatterv */
/* the counts of one v-case, in bytes */
struct VCase {
    std::vector<uint64_t> cnt;
    uint64_t              B        = 0;
    bool                  fits     = true;
    int                   odd_rank = -1; /* scatterv: its dst disagrees */
    int64_t               odd_by   = 0;  /* ... by this many bytes      */
};

static uint64_t stride_sum(const std::vector<uint64_t> &cnt)
{
    uint64_t s = 0;
    for (auto c : cnt) {
        s += fused_plan_stride(c);
    }
    return s;
}

/* kind 0: seeded counts with a zero; 1: the root's own count is zero; 2: one
 * rank is the only non-zero one. B leaves room for them (scatterv: the sum,
 * which is no less than gatherv's largest block). */
static VCase seeded_case(Rng &g, int n, int root, size_t esz, int kind)
{
    VCase v;
    v.cnt.assign((size_t)n, 0);
    if (kind == 2) {
        v.cnt[g.below((uint32_t)n)] = (1 + g.below(300)) * esz;
    } else {
        for (auto &c : v.cnt) {
            c = pick_count(g) * esz;
        }
        v.cnt[g.below((uint32_t)n)]      = 0;
        v.cnt[(size_t)((root + 1) % n)] = 7 * esz; /* one non-zero */
        if (kind == 1) {
            v.cnt[(size_t)root] = 0;
        }
    }
    v.B = stride_sum(v.cnt) + 16 * g.below(4);
    return v;
}

static bool sim_gatherv(Rng &g, int n, int root, size_t esz, const VCase &v,
                        bool ip)
{
    std::vector<uint64_t> dsp;
    const uint64_t        ext = layout(g, n, v.cnt, &dsp, esz);
    std::vector<Rank>     rk((size_t)n);
    for (int r = 0; r < n; r++) {
        Rank          &k       = rk[(size_t)r];
        const bool     mine_ip = ip && r == root;
        const uint64_t mine    = v.cnt[(size_t)r];
        /* counts and displacements exist at the root only */
        CHECK(fused_plan_init_rooted_v(
                  &k.plan, FUSED_GATHERV, n, r, root,
                  r == root ? v.cnt.data() : nullptr,
                  r == root ? dsp.data() : nullptr, r == root ? 0 : mine,
                  v.B, esz, ip),
              "plan refused");
        CHECK(r != root || k.plan.fits_local == v.fits, "root's fits_local");
        CHECK(k.plan.n_cells ==
                  ((mine && mine <= v.B && !mine_ip &&
                    (r != root || v.fits))
                       ? 1
                       : 0),
              "gatherv cells");
        k.src.init(mine_ip ? 0 : mine);
        k.dst.init(r == root ? ext : 32);
        k.expect_init();
        for (uint64_t i = 0; !mine_ip && i < mine; i++) {
            k.src.at(i) = val(r, i);
        }
        for (int s = 0; r == root && s < n; s++) {
            const bool kept = ip && s == root;
            for (uint64_t i = 0; i < v.cnt[(size_t)s]; i++) {
                if (kept) {
                    k.dst.at(dsp[(size_t)s] + i) = val(s, i);
                }
                k.want(dsp[(size_t)s] + i, val(s, i),
                       kept ? kKept : kWritten);
            }
        }
    }
    bool fits = false;
    if (!run(rk, n, root, true, &fits)) {
        return false;
    }
    CHECK(fits == v.fits, "verdict");
    return true;
}

static bool sim_scatterv(Rng &g, int n, int root, size_t esz, const VCase &v,
                         bool ip)
{
    std::vector<uint64_t> dsp;
    const uint64_t        ext = layout(g, n, v.cnt, &dsp, esz);
    std::vector<Rank>     rk((size_t)n);
    for (int r = 0; r < n; r++) {
        Rank      &k       = rk[(size_t)r];
        const bool mine_ip = ip && r == root;
        uint64_t   mine    = v.cnt[(size_t)r];
        if (r == v.odd_rank) {
            mine = (uint64_t)((int64_t)mine + v.odd_by);
        }
        CHECK(fused_plan_init_rooted_v(
                  &k.plan, FUSED_SCATTERV, n, r, root,
                  r == root ? v.cnt.data() : nullptr,
                  r == root ? dsp.data() : nullptr, mine_ip ? 0 : mine, v.B,
                  esz, ip),
              "plan refused");
        CHECK(r != root || k.plan.fits_local == v.fits, "root's fits_local");
        if (r == root && v.fits) {
            int cells = 0;
            for (int d = 0; d < n; d++) {
                cells += v.cnt[(size_t)d] && !(ip && d == root);
            }
            CHECK(k.plan.n_cells == cells, "scatterv cells");
        }
        k.src.init(r == root ? ext : 0);
        k.dst.init(mine_ip ? 0 : mine);
        k.expect_init();
        for (int d = 0; r == root && d < n; d++) {
            for (uint64_t i = 0; i < v.cnt[(size_t)d]; i++) {
                k.src.at(dsp[(size_t)d] + i) = val(d, i);
            }
        }
        const uint64_t got = std::min(mine, v.cnt[(size_t)r]);
        for (uint64_t i = 0; !mine_ip && i < got; i++) {
            k.want(i, val(r, i));
        }
    }
    std::vector<uint8_t> src_before = rk[(size_t)root].src.b;
    bool                 fits       = false;
    if (!run(rk, n, root, true, &fits)) {
        return false;
    }
    CHECK(fits == v.fits, "verdict");
    CHECK(rk[(size_t)root].src.b == src_before, "the root's src changed");
    return true;
}

/* the cases at the bound. which: 0 = a block of exactly B at `at`, 1 = B plus
 * one element there; scatterv only: 2 = a stride sum of exactly B, 3 = a sum
 * of B + 16. For gatherv the other ranks hold small blocks, for scatterv
 * (which 0, 1) nothing, since there the sum counts. */
static VCase bound_case(int n, int at, size_t esz, bool scatter, int which)
{
    VCase v;
    v.B = 4096;
    v.cnt.assign((size_t)n, scatter ? 0 : 7 * esz);
    if (which <= 1) {
        v.cnt[(size_t)at] = v.B + (which ? esz : 0);
        v.fits            = which == 0;
    } else {
        /* n - 1 blocks of 7 elements, whose strides are no multiple of
         * their lengths, and one block that fills the rest exactly */
        v.cnt.assign((size_t)n, 7 * esz);
        v.cnt[(size_t)at] = 0;
        v.cnt[(size_t)at] = v.B - stride_sum(v.cnt) + (which == 3 ? 16 : 0);
        v.fits            = which == 2;
    }
    return v;
}

static bool refusals()
{
    FusedPlan      p;
    const uint64_t c4[4] = {64, 0, 6, 64}, z4[4] = {0, 0, 0, 0},
                   d4[4] = {0, 64, 64, 80};
    CHECK(!fused_plan_init(&p, FUSED_GATHER, 1, 0, 0, 64, 2, false), "n 1");
    CHECK(!fused_plan_init(&p, FUSED_SCATTER, 9, 0, 0, 64, 2, false), "n 9");
    CHECK(!fused_plan_init(&p, FUSED_GATHER, 4, 4, 0, 64, 2, false), "rank");
    CHECK(!fused_plan_init(&p, FUSED_SCATTER, 4, 0, 4, 64, 2, false), "root");
    CHECK(!fused_plan_init(&p, FUSED_GATHER, 4, 0, 0, 63, 2, false), "elem");
    CHECK(!fused_plan_init(&p, FUSED_GATHERV, 4, 0, 0, 64, 2, false),
          "a v-form through fused_plan_init");
    for (FusedColl c : {FUSED_GATHERV, FUSED_SCATTERV}) {
        CHECK(fused_plan_init_rooted_v(&p, c, 4, 0, 0, c4, d4, 64, 64, 2,
                                       false),
              "a plain plan refused");
        CHECK(!fused_plan_init_rooted_v(&p, c, 1, 0, 0, c4, d4, 64, 64, 2,
                                        false),
              "n 1");
        CHECK(!fused_plan_init_rooted_v(&p, c, 9, 0, 0, c4, d4, 64, 64, 2,
                                        false),
              "n 9");
        CHECK(!fused_plan_init_rooted_v(&p, c, 4, -1, 0, c4, d4, 64, 64, 2,
                                        false),
              "rank");
        CHECK(!fused_plan_init_rooted_v(&p, c, 4, 0, 4, c4, d4, 64, 64, 2,
                                        false),
              "root");
        CHECK(!fused_plan_init_rooted_v(&p, c, 4, 0, 0, c4, d4, 64, 64, 4,
                                        false),
              "a count that is no multiple of the element");
        CHECK(!fused_plan_init_rooted_v(&p, c, 4, 1, 0, nullptr, nullptr, 6,
                                        64, 4, false),
              "a length that is no multiple of the element");
        CHECK(!fused_plan_init_rooted_v(&p, c, 4, 0, 0, z4, d4, 0, 64, 2,
                                        false),
              "all counts zero at the root");
        CHECK(!fused_plan_init_rooted_v(&p, c, 4, 0, 0, c4, d4, 64, 0, 2,
                                        false),
              "B 0");
        CHECK(!fused_plan_init_rooted_v(&p, c, 4, 0, 0, nullptr, nullptr, 64,
                                        64, 2, false),
              "a root without counts");
        /* a non-root needs no counts, and a zero length is a plan */
        CHECK(fused_plan_init_rooted_v(&p, c, 4, 1, 0, nullptr, nullptr, 0,
                                       64, 2, false),
              "a non-root with nothing refused");
    }
    CHECK(!fused_plan_init_rooted_v(&p, FUSED_ALLGATHERV, 4, 0, 0, c4, d4, 64,
                                    64, 2, false),
          "another type through fused_plan_init_rooted_v");
    /* B from the knob: the header off, rounded down to 16 */
    CHECK(kFusedRootedHdr == 144, "header size");
    CHECK(fused_plan_rooted_v_bound(8192) == 8048, "B of 8k");
    CHECK(fused_plan_rooted_v_bound(524288) == 524144, "B of 512k");
    CHECK(fused_plan_rooted_v_bound(160) == 16, "B of 160");
    CHECK(fused_plan_rooted_v_bound(159) == 0, "B of 159");
    CHECK(fused_plan_rooted_v_bound(0) == 0, "B of 0");
    CHECK(fused_plan_scratch_bytes(FUSED_GATHER, 4, 17) == 32 &&
              fused_plan_scratch_bytes(FUSED_SCATTER, 4, 17) == 128,
          "scratch_bytes of gather / scatter");
    /* a table entry that leaves the area copies nothing */
    uint64_t off, len;
    CHECK(fused_plan_init_rooted_v(&p, FUSED_SCATTERV, 4, 0, 0, c4, d4, 64,
                                   256, 2, false),
          "plan refused");
    CHECK(fused_plan_rooted_v_verdict(p, 3, 64, &off, &len) && len == 64 &&
              off == p.tab_off[3],
          "a good entry");
    p.tab_len[3] = 256;
    CHECK(fused_plan_rooted_v_verdict(p, 3, 1024, &off, &len) && len == 0,
          "an entry past the area copies");
    p.tab_len[3] = 64;
    p.tab_off[3] = 8;
    CHECK(fused_plan_rooted_v_verdict(p, 3, 64, &off, &len) && len == 0,
          "an entry on the header copies");
    p.tab_off[3] = kFusedRootedHdr + 8;
    CHECK(fused_plan_rooted_v_verdict(p, 3, 64, &off, &len) && len == 0,
          "a misaligned entry copies");
    return true;
}

int main()
{
    const size_t   eszs[]  = {1, 2, 4, 8, 16};
    const uint64_t elems[] = {1, 0 /* exactly 16 bytes */, 7, 999};
    uint64_t       sims    = 0;
#define SIM(name, call)                                                      \
    do {                                                                     \
        if (!(call)) {                                                       \
            printf("FAIL %s n=%d root=%d esz=%zu: %s\n", name, n, root,      \
                   esz, g_what);                                             \
            return 1;                                                        \
        }                                                                    \
        sims++;                                                              \
    } while (0)
    for (int n = 2; n <= kFusedMaxRanks; n++) {
        for (int root = 0; root < n; root++) {
            for (size_t esz : eszs) {
                Rng g{(uint64_t)n * 1000003 + (uint64_t)root * 101 + esz};
                for (uint64_t e : elems) {
                    const uint64_t el = e ? e : 16 / esz;
                    for (int ip = 0; ip < 2; ip++) {
                        SIM("gather", sim_gather(n, root, esz, el, ip));
                        SIM("scatter", sim_scatter(n, root, esz, el, ip));
                    }
                }
                for (int kind = 0; kind < 3; kind++) {
                    for (int ip = 0; ip < 2; ip++) {
                        VCase v = seeded_case(g, n, root, esz, kind);
                        SIM("gatherv", sim_gatherv(g, n, root, esz, v, ip));
                        v = seeded_case(g, n, root, esz, kind);
                        SIM("scatterv", sim_scatterv(g, n, root, esz, v, ip));
                    }
                }
                /* at the bound: at the root's own index and at another's */
                const int other = (root + 1 + (int)g.below((uint32_t)n - 1)) % n;
                for (int at : {root, other}) {
                    for (int which = 0; which < 2; which++) {
                        SIM("gatherv at the bound",
                            sim_gatherv(g, n, root, esz,
                                        bound_case(n, at, esz, false, which),
                                        false));
                    }
                    for (int which = 0; which < 4; which++) {
                        SIM("scatterv at the bound",
                            sim_scatterv(g, n, root, esz,
                                         bound_case(n, at, esz, true, which),
                                         false));
                    }
                }
                /* the root's own block of exactly B, in place: not staged,
                 * it fits all the same */
                SIM("gatherv at the bound, in place",
                    sim_gatherv(g, n, root, esz,
                                bound_case(n, root, esz, false, 0), true));
                /* a non-root whose dst is shorter, then longer, than what
                 * the root sends it */
                for (int64_t by : {-(int64_t)esz, (int64_t)(3 * esz)}) {
                    VCase v = seeded_case(g, n, root, esz, 0);
                    v.odd_rank = other;
                    v.odd_by   = by;
                    v.cnt[(size_t)other] = 40 * esz;
                    v.B                  = stride_sum(v.cnt);
                    SIM("scatterv, lengths disagree",
                        sim_scatterv(g, n, root, esz, v, false));
                }
            }
        }
    }
    if (!refusals()) {
        printf("FAIL refusals: %s\n", g_what);
        return 1;
    }
    printf("FUSED_PLAN_ROOTED_OK sims=%llu\n", (unsigned long long)sims);
    return 0;
}
