/* Host-only check of src/tl/cdna4/ring_plan.h: all ranks of a multi-ring
 * reduce_scatter / allgather / allreduce simulated on host memory with
 * integer payloads, launches executed one at a time in randomised orders
 * that respect the gate.
 *
 * Payload of rank s at element e of the n-block vector: a contribution word
 * with 1 in byte lane s, and an id word e + 1. After a reduction every byte
 * lane 0..n-1 of the contribution word must be exactly 1 (every rank once,
 * none twice) and the id word must be n * (e + 1) (the right element).
 *
 * Every outbox half remembers the launch index that last wrote it. A reader
 * at launch g must find g - 1 there; anything else means the half was
 * overwritten before its reader's launch (or read before it was written).
 * With the right-neighbour clause of the gate dropped that check must fire
 * for some n >= 3: the clause is necessary. */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../src/tl/cdna4/ring_plan.h"

using namespace ucc;

struct Val {
    uint64_t contrib = 0, id = 0;
};
static inline Val operator+(Val a, Val b)
{
    return Val{a.contrib + b.contrib, a.id + b.id};
}
static inline bool operator==(Val a, Val b)
{
    return a.contrib == b.contrib && a.id == b.id;
}

struct Rank {
    RingPlan         plan;
    std::vector<Val> buf;       /* src and dst; aliased when in place */
    size_t           src0 = 0, dst0 = 0; /* base indices into buf       */
    std::vector<Val> box[2];
    int64_t          box_gen[2] = {-1, -1};
    uint64_t         done = 0;  /* completed launches                   */
};

struct Result {
    bool     ok = true;        /* placement and contributions          */
    uint64_t overwrites = 0;   /* reads that found the wrong generation */
    uint64_t bounds = 0;       /* descriptor outside its buffer          */
};

static Val src_val(int s, uint64_t e)
{
    return Val{1ull << (8 * s), e + 1};
}

static Result simulate(int n, int nrings_knob, RingColl coll, bool inplace,
                       uint64_t count, size_t dtsz, size_t accsz,
                       size_t chunk, uint32_t seed, bool with_right,
                       uint64_t *launches_out)
{
    Result            res;
    std::vector<Rank> rk(n);
    /* per-rank element counts of the src and dst buffers */
    const uint64_t vec = coll == RING_ALLREDUCE ? count : count * n;
    for (int r = 0; r < n; r++) {
        Rank &R = rk[r];
        if (!ring_plan_init(&R.plan, n, r, nrings_knob, coll, inplace, count,
                            dtsz, accsz, chunk)) {
            res.ok = false;
            return res;
        }
        const uint64_t src_n = coll == RING_ALLGATHER ? count : vec;
        const uint64_t dst_n = coll == RING_REDUCE_SCATTER ? count : vec;
        if (!inplace) {
            R.buf.assign(src_n + dst_n, Val{});
            R.src0 = 0;
            R.dst0 = src_n;
        } else if (coll == RING_ALLREDUCE) {
            R.buf.assign(vec, Val{});
        } else if (coll == RING_REDUCE_SCATTER) {
            R.buf.assign(vec, Val{});
            R.dst0 = (size_t)r * count; /* my block of the vector */
        } else {
            R.buf.assign(vec, Val{});
            R.src0 = (size_t)r * count;
        }
        for (uint64_t e = 0; e < src_n; e++) {
            /* allgather: my block's elements carry their global index */
            const uint64_t ge =
                coll == RING_ALLGATHER ? (uint64_t)r * count + e : e;
            R.buf[R.src0 + e] = src_val(r, ge);
        }
        R.box[0].assign(R.plan.cell, Val{});
        R.box[1].assign(R.plan.cell, Val{});
    }
    const uint64_t total = ring_plan_launches(rk[0].plan);
    *launches_out        = total;
    std::mt19937 rng(seed);
    for (;;) {
        std::vector<int> ready;
        bool             all_done = true;
        for (int r = 0; r < n; r++) {
            if (rk[r].done >= total) {
                continue;
            }
            all_done = false;
            int  nb[2 * kRingMaxRings];
            int  k  = ring_plan_neighbours(rk[r].plan, nb, with_right);
            bool go = true;
            for (int i = 0; i < k; i++) {
                go = go && rk[nb[i]].done >= rk[r].done;
            }
            if (go) {
                ready.push_back(r);
            }
        }
        if (all_done) {
            break;
        }
        if (ready.empty()) {
            fprintf(stderr, "deadlock: n=%d coll=%d\n", n, (int)coll);
            res.ok = false;
            return res;
        }
        const int r = ready[rng() % ready.size()];
        Rank     &R = rk[r];
        const uint64_t g = R.done;
        const uint64_t f = g / (uint64_t)R.plan.L;
        const int      j = (int)(g % (uint64_t)R.plan.L);
        RingLaunch     l;
        ring_plan_launch(R.plan, f, j, &l);
        if (l.out_parity != (int)(g & 1) || l.in_parity != (int)((g + 1) & 1)) {
            res.ok = false;
        }
        const size_t in_sz  = l.in_acc ? accsz : dtsz;
        const size_t out_sz = l.out_acc ? accsz : dtsz;
        /* lanes of one launch must not overlap in the outbox */
        for (int a = 0; a < l.npieces; a++) {
            for (int b = a + 1; b < l.npieces; b++) {
                const RingPieceDesc &x = l.p[a], &y = l.p[b];
                if (x.count && y.count && x.box_off < y.box_off + y.count &&
                    y.box_off < x.box_off + x.count) {
                    res.bounds++;
                }
            }
        }
        for (int k = 0; k < l.npieces; k++) {
            const RingPieceDesc &d = l.p[k];
            if (d.count == 0) {
                continue;
            }
            const uint64_t src_n = coll == RING_ALLGATHER ? count : vec;
            const uint64_t dst_n = coll == RING_REDUCE_SCATTER ? count : vec;
            if ((d.box_off + d.count) * (l.use_in ? in_sz : 0) > chunk ||
                (d.box_off + d.count) * (l.use_out ? out_sz : 0) > chunk ||
                d.box_off + d.count > R.plan.cell ||
                ((l.in_from_src || l.use_local) &&
                 d.src_off + d.count > src_n) ||
                (l.use_dst && d.dst_off + d.count > dst_n) ||
                (d.box_off * dtsz) % 16 != 0) {
                res.bounds++;
                continue;
            }
            if (l.use_in && rk[d.left].box_gen[l.in_parity] != (int64_t)g - 1) {
                res.overwrites++;
            }
            for (uint64_t i = 0; i < d.count; i++) {
                Val acc;
                if (l.in_from_src) {
                    acc = R.buf[R.src0 + d.src_off + i];
                } else {
                    acc = rk[d.left].box[l.in_parity][d.box_off + i];
                    if (l.use_local) {
                        acc = acc + R.buf[R.src0 + d.src_off + i];
                    }
                }
                if (l.use_out) {
                    R.box[l.out_parity][d.box_off + i] = acc;
                }
                if (l.use_dst) {
                    R.buf[R.dst0 + d.dst_off + i] = acc;
                }
            }
        }
        if (l.use_out) {
            R.box_gen[l.out_parity] = (int64_t)g;
        }
        R.done++;
    }
    /* final placement */
    uint64_t all = 0;
    for (int s = 0; s < n; s++) {
        all += 1ull << (8 * s);
    }
    for (int r = 0; r < n; r++) {
        const Rank &R = rk[r];
        if (coll == RING_ALLGATHER) {
            for (uint64_t e = 0; e < vec; e++) {
                res.ok = res.ok && R.buf[R.dst0 + e] ==
                                       src_val((int)(e / count), e);
            }
        } else {
            const uint64_t lo = coll == RING_ALLREDUCE ? 0 : r * count;
            const uint64_t hi = coll == RING_ALLREDUCE ? vec : lo + count;
            for (uint64_t e = lo; e < hi; e++) {
                res.ok = res.ok && R.buf[R.dst0 + (e - lo)] ==
                                       Val{all, (uint64_t)n * (e + 1)};
            }
        }
    }
    return res;
}

static int phi(int n)
{
    int c = 0;
    for (int q = 1; q < n; q++) {
        c += ring_gcd(q, n) == 1;
    }
    return c;
}

int main()
{
    int failures = 0;
    /* stride sets the schedule promises */
    {
        const int want[][5] = {{2, 1, 0, 0, 0}, {3, 1, 2, 0, 0},
                               {4, 1, 3, 0, 0}, {6, 1, 5, 0, 0},
                               {8, 1, 3, 5, 7}};
        for (auto &w : want) {
            int q[kRingMaxRings] = {};
            int r = ring_strides(w[0], kRingAutoRings, q);
            int e = 0;
            while (e < 4 && w[1 + e]) {
                e++;
            }
            bool ok = r == e;
            for (int i = 0; i < e && ok; i++) {
                ok = q[i] == w[1 + i];
            }
            if (!ok) {
                fprintf(stderr, "stride set of n=%d wrong\n", w[0]);
                failures++;
            }
        }
    }
    const size_t   dtsz = 2, accsz = 4; /* bf16 travelling as f32 */
    const size_t   tiny = 256;          /* chunk: cell = 64 elements */
    uint64_t       sims = 0, gate_hits = 0;
    const RingColl colls[3] = {RING_REDUCE_SCATTER, RING_ALLGATHER,
                               RING_ALLREDUCE};
    for (int n = 2; n <= 8; n++) {
        int maxr = phi(n) < kRingMaxRings ? phi(n) : kRingMaxRings;
        for (int R = 0; R <= maxr; R++) { /* 0 = auto */
            for (RingColl coll : colls) {
                /* per-rank counts; allreduce gets n times that (+ a rest) */
                const uint64_t counts[4] = {1, (uint64_t)n - 1, 13,
                                            2 * 64 + 5};
                for (uint64_t c : counts) {
                    for (int inplace = 0; inplace < 2; inplace++) {
                        uint64_t cnt = c;
                        if (coll == RING_ALLREDUCE) {
                            /* 1, n-1 as they are; the others: a vector
                             * whose blocks have c elements and more */
                            cnt = c <= (uint64_t)n ? c
                                  : c == 13        ? 128 * n + 13
                                                   : (2 * 64 + 5) * n + 128 + 3;
                        }
                        const size_t chunk =
                            c == 2 * 64 + 5 ? tiny : (size_t)8192;
                        for (uint32_t seed = 1; seed <= 3; seed++) {
                            uint64_t L  = 0;
                            Result   rs = simulate(
                                n, R, coll, inplace, cnt, dtsz, accsz, chunk,
                                seed * 7919u + n, true, &L);
                            sims++;
                            if (!rs.ok || rs.overwrites || rs.bounds) {
                                fprintf(stderr,
                                        "FAIL n=%d R=%d coll=%d count=%llu "
                                        "inplace=%d seed=%u ok=%d ow=%llu "
                                        "bounds=%llu\n",
                                        n, R, (int)coll,
                                        (unsigned long long)cnt, inplace,
                                        seed, (int)rs.ok,
                                        (unsigned long long)rs.overwrites,
                                        (unsigned long long)rs.bounds);
                                failures++;
                            }
                            if (c == 2 * 64 + 5 &&
                                L < 3 * (uint64_t)(coll == RING_ALLREDUCE
                                                       ? 2 * n - 1
                                                       : n)) {
                                fprintf(stderr, "n=%d coll=%d: %llu launches "
                                        "are fewer than 3 fragments\n", n,
                                        (int)coll, (unsigned long long)L);
                                failures++;
                            }
                        }
                    }
                }
            }
        }
    }
    /* the right-neighbour clause is necessary */
    for (int n = 3; n <= 8; n++) {
        for (uint32_t seed = 1; seed <= 20; seed++) {
            uint64_t L  = 0;
            Result   rs = simulate(n, 1, RING_ALLREDUCE, false,
                                   (2 * 64 + 5) * n, dtsz, accsz, tiny, seed,
                                   false, &L);
            gate_hits += rs.overwrites > 0;
        }
    }
    if (gate_hits == 0) {
        fprintf(stderr, "gate without the right-neighbour clause: no "
                "overwrite reported for any n >= 3\n");
        failures++;
    }
    /* a chunk below one 16-byte pack of the accumulator is refused */
    {
        RingPlan p;
        if (ring_plan_init(&p, 4, 0, 0, RING_ALLREDUCE, false, 100, 2, 4,
                           16) ||
            ring_plan_init(&p, 9, 0, 0, RING_ALLREDUCE, false, 100, 2, 4,
                           4096) ||
            !ring_plan_init(&p, 4, 0, 0, RING_ALLREDUCE, false, 100, 2, 4,
                            32)) {
            fprintf(stderr, "ring_plan_init accept/refuse wrong\n");
            failures++;
        }
    }
    printf("sims=%llu gate_hits=%llu failures=%d\n",
           (unsigned long long)sims, (unsigned long long)gate_hits,
           failures);
    if (failures == 0) {
        printf("RING_PLAN_OK\n");
    }
    return failures ? 1 : 0;
}
