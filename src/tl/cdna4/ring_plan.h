/* Schedule arithmetic of tl/cdna4's host-gated multi-ring reduce_scatter,
 * allgather and allreduce (RingTask in tl_cdna4.cc). Host only, no HIP: a
 * pure function of (n, rank, nrings, coll, count, dtype size, accumulator
 * size, chunk) that says, for every fragment and launch, what one
 * ec_hip::ring_step launch is given. tests/native/test_ring_plan.cc runs it
 * for all ranks on host memory.
 *
 * Rings. Ring k has stride q_k, the k-th smallest q in [1, n) with
 * gcd(q, n) = 1. In ring k rank r reads from left = (r - q_k) mod n and is
 * read by right = (r + q_k) mod n, so the directed link r -> r + q carries
 * the ring of stride q only: the rings are link-disjoint.
 * R = min(knob ? knob : 4, phi(n), kRingMaxRings).
 *
 * Blocks. Block b is the part owned by rank b: `count` elements each for
 * reduce_scatter and allgather; for allreduce per = floor(count / n) rounded
 * down to 256 / dtsize elements, the last block takes the rest (StagedTask's
 * split; per may be 0).
 *
 * Pieces. Ring k carries piece k of every block. Piece k of a block of c
 * elements is [min(k * psz, c), min((k + 1) * psz, c)), the last piece runs
 * to c; psz = floor(bmax / R) rounded down to 16 bytes, bmax the largest
 * block. One psz for all blocks keeps piece k of ANY block inside lane
 * [k * psz, (k + 1) * psz): in one launch the rings handle different blocks
 * and share one outbox, and allreduce's last block is longer than the
 * others, so a per-block cut would make their pieces overlap there.
 *
 * Fragments. Fragment f covers [f * cell, (f + 1) * cell) of every block;
 * cell = chunk / max(accsize, dtsize) elements rounded down to 16 bytes. A
 * piece lies in the outbox at its element offset from the fragment start,
 * scaled by the size of the stored type.
 *
 * Launches. L per fragment: n for reduce_scatter and allgather, 2n - 1 for
 * allreduce. Global index g = f * L + j; launch g writes outbox parity g & 1
 * and reads the left neighbours' parity (g - 1) & 1.
 *   RS launch j: block B = (r + (n - 1 - j) * q) mod n.
 *     j = 0           src[B] -> outbox, type T
 *     0 < j < n - 1   op(left's outbox, src[B]) -> outbox, accumulator type
 *     j = n - 1       B = r: -> dst, alpha applied, rounded once; allreduce
 *                     also stores those bits, type T, in the outbox
 *   AG launch t (1 <= t < n): block G = (r - t * q) mod n from left's outbox
 *     -> dst, and -> outbox unless t = n - 1.
 *   allgather launch 0: my src -> outbox, and -> my dst block unless in
 *     place.
 *
 * Gate. Before launch g every ring neighbour (left and right, all rings)
 * has published >= g, i.e. completed its launches 0..g-1. Left's count
 * covers the data; right's covers that its launch g - 1 was the last reader
 * of the outbox half that launch g overwrites. */
#ifndef UCC_AMD_RING_PLAN_H_
#define UCC_AMD_RING_PLAN_H_

#include <cstddef>
#include <cstdint>

namespace ucc {

constexpr int kRingMaxRanks = 8;
constexpr int kRingMaxRings = 4;
constexpr int kRingAutoRings = 4;

enum RingColl { RING_REDUCE_SCATTER = 0, RING_ALLGATHER = 1,
                RING_ALLREDUCE = 2 };

struct RingPlan {
    int      n = 0, rank = 0, nrings = 0;
    int      q[kRingMaxRings] = {};
    RingColl coll = RING_ALLREDUCE;
    bool     inplace = false;
    uint64_t boff[kRingMaxRanks] = {}; /* block start, elements            */
    uint64_t bcnt[kRingMaxRanks] = {}; /* block length, elements           */
    uint64_t bmax = 0;                 /* longest block                    */
    uint64_t psz = 0;                  /* piece lane width, elements       */
    uint64_t cell = 0;                 /* fragment width, elements         */
    uint64_t nfrags = 0;
    size_t   dtsz = 0, accsz = 0;
    int      L = 0;                    /* launches per fragment            */
};

/* what ring k of one launch is given; offsets count elements */
struct RingPieceDesc {
    uint64_t count = 0;
    int      block = 0;
    int      left = 0;      /* whose outbox `in` is (unless in_from_src)   */
    uint64_t box_off = 0;   /* in (outbox) and out: from the outbox start  */
    uint64_t src_off = 0;   /* local, or in when in_from_src: from the src
                               base (reduce_scatter, allreduce: the n-block
                               vector; allgather: my block)                */
    uint64_t dst_off = 0;   /* from the dst base (reduce_scatter: my block;
                               allgather, allreduce: the n-block vector)   */
};

struct RingLaunch {
    int  npieces = 0;
    bool in_from_src = false; /* in = src + src_off, a byte copy          */
    bool use_in = false;      /* in = left's outbox + box_off             */
    bool use_local = false;   /* local = src + src_off                    */
    bool use_out = false, use_dst = false;
    bool final_rs = false;    /* dst gets alpha * acc                     */
    int  in_acc = 0, out_acc = 0;
    int  in_parity = 0, out_parity = 0;
    RingPieceDesc p[kRingMaxRings];
};

static inline int ring_gcd(int a, int b)
{
    while (b) {
        int t = a % b;
        a     = b;
        b     = t;
    }
    return a;
}

/* strides of the first min(want, phi(n), kRingMaxRings) rings */
static inline int ring_strides(int n, int want, int *q)
{
    int r = 0;
    for (int s = 1; s < n && r < want && r < kRingMaxRings; s++) {
        if (ring_gcd(s, n) == 1) {
            q[r++] = s;
        }
    }
    return r;
}

/* count: elements per rank for reduce_scatter and allgather, of the whole
 * vector for allreduce. nrings_knob 0 = auto. false: not expressible (rank
 * count, sizes, or a chunk too small for one 16-byte pack per fragment). */
static inline bool ring_plan_init(RingPlan *p, int n, int rank,
                                  int nrings_knob, RingColl coll,
                                  bool inplace, uint64_t count, size_t dtsz,
                                  size_t accsz, size_t chunk)
{
    if (n < 2 || n > kRingMaxRanks || rank < 0 || rank >= n || dtsz == 0 ||
        dtsz > 16 || (dtsz & (dtsz - 1)) || accsz < dtsz ||
        (accsz & (accsz - 1)) || nrings_knob < 0) {
        return false;
    }
    *p         = RingPlan{};
    p->n       = n;
    p->rank    = rank;
    p->coll    = coll;
    p->inplace = inplace;
    p->dtsz    = dtsz;
    p->accsz   = accsz;
    p->nrings  = ring_strides(n, nrings_knob ? nrings_knob : kRingAutoRings,
                              p->q);
    const uint64_t pack = 16 / dtsz; /* elements per 16 bytes */
    if (coll == RING_ALLREDUCE) {
        const uint64_t gran = 256 / dtsz;
        const uint64_t per  = (count / (uint64_t)n) / gran * gran;
        for (int b = 0; b < n; b++) {
            p->boff[b] = (uint64_t)b * per;
            p->bcnt[b] = b == n - 1 ? count - p->boff[b] : per;
        }
    } else {
        for (int b = 0; b < n; b++) {
            p->boff[b] = (uint64_t)b * count;
            p->bcnt[b] = count;
        }
    }
    for (int b = 0; b < n; b++) {
        p->bmax = p->bcnt[b] > p->bmax ? p->bcnt[b] : p->bmax;
    }
    p->psz  = (p->bmax / (uint64_t)p->nrings) / pack * pack;
    p->cell = (uint64_t)(chunk / accsz) / pack * pack;
    if (p->cell == 0) {
        return false;
    }
    p->nfrags = (p->bmax + p->cell - 1) / p->cell;
    if (p->nfrags == 0) {
        p->nfrags = 1;
    }
    p->L = coll == RING_ALLREDUCE ? 2 * n - 1 : n;
    return true;
}

static inline uint64_t ring_plan_launches(const RingPlan &p)
{
    return p.nfrags * (uint64_t)p.L;
}

/* the ranks the gate of `rank` looks at: left and right of every ring,
 * each once; with_right = false drops the right-neighbour clause (only the
 * plan test does that, to show that the clause is needed) */
static inline int ring_plan_neighbours(const RingPlan &p, int *out,
                                       bool with_right = true)
{
    int k = 0;
    for (int r = 0; r < p.nrings; r++) {
        const int cand[2] = {((p.rank - p.q[r]) % p.n + p.n) % p.n,
                             (p.rank + p.q[r]) % p.n};
        for (int c = 0; c < (with_right ? 2 : 1); c++) {
            bool dup = false;
            for (int i = 0; i < k; i++) {
                dup |= out[i] == cand[c];
            }
            if (!dup) {
                out[k++] = cand[c];
            }
        }
    }
    return k;
}

/* launch j (0 <= j < L) of fragment f */
static inline void ring_plan_launch(const RingPlan &p, uint64_t f, int j,
                                    RingLaunch *l)
{
    const int n = p.n, r = p.rank;
    *l          = RingLaunch{};
    l->npieces  = p.nrings;
    const uint64_t g = f * (uint64_t)p.L + (uint64_t)j;
    l->out_parity    = (int)(g & 1);
    l->in_parity     = (int)((g + 1) & 1);
    const bool rs = p.coll != RING_ALLGATHER && j < n;
    int        t  = 0; /* allgather-phase step */
    if (rs) {
        if (j == 0) {
            l->in_from_src = true;
            l->use_out     = true;
        } else {
            l->use_in    = true;
            l->use_local = true;
            l->in_acc    = j >= 2;
            if (j < n - 1) {
                l->use_out = true;
                l->out_acc = 1;
            } else {
                l->use_dst  = true;
                l->final_rs = true;
                l->use_out  = p.coll == RING_ALLREDUCE;
            }
        }
    } else {
        t = p.coll == RING_ALLGATHER ? j : j - (n - 1);
        if (t == 0) {
            l->in_from_src = true;
            l->use_out     = true;
            l->use_dst     = !p.inplace;
        } else {
            l->use_in  = true;
            l->use_dst = true;
            l->use_out = t < n - 1;
        }
    }
    const uint64_t fb = f * p.cell;
    const uint64_t fe = fb + p.cell < p.bmax ? fb + p.cell : p.bmax;
    for (int k = 0; k < p.nrings; k++) {
        RingPieceDesc &d = l->p[k];
        const int      q = p.q[k];
        d.left           = ((r - q) % n + n) % n;
        d.block          = rs ? (r + (n - 1 - j) * q) % n
                              : ((r - t * q) % n + n) % n;
        const uint64_t c  = p.bcnt[d.block];
        uint64_t       pb = (uint64_t)k * p.psz;
        uint64_t       pe = k == p.nrings - 1 ? c : pb + p.psz;
        pb                = pb < c ? pb : c;
        pe                = pe < c ? pe : c;
        const uint64_t s  = pb > fb ? pb : fb;
        const uint64_t e  = pe < fe ? pe : fe;
        if (e <= s) {
            continue; /* count 0 */
        }
        d.count   = e - s;
        d.box_off = s - fb;
        d.src_off = (p.coll == RING_ALLGATHER ? 0 : p.boff[d.block]) + s;
        d.dst_off = (p.coll == RING_REDUCE_SCATTER ? 0 : p.boff[d.block]) + s;
    }
}

} // namespace ucc

#endif
