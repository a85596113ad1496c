/* Per-pair mailbox (src/tl/cdna4/p2p_mbox.h) across three processes, no
 * HIP: attach-before-create, ring-full back-pressure, wrap-around past the
 * ring depth, per-pair independence and the error-status ack. Also the
 * `make asan` payload for the mailbox. */
#include <cstdio>
#include <cstdlib>
#include <new>
#include <sched.h>
#include <sys/wait.h>

#include "../../src/tl/cdna4/p2p_mbox.h"

using namespace ucc;

static constexpr uint32_t kRanks = 3;
static constexpr uint32_t kD     = 4;          /* ring depth under test */
static constexpr uint64_t kN     = 3 * kD + 3; /* wraps the ring 3x     */
static constexpr uint64_t kErrSeq = 5;
static constexpr int32_t  kErrSt  = (int32_t)UCC_ERR_INVALID_PARAM;

/* process-shared coordination page (mapped before fork) */
struct Shared {
    std::atomic<int> full; /* rank 0 filled ring 0->1, nothing acked yet */
    std::atomic<int> go;   /* rank 2 saw 2->1 finish while 0->1 is stuck */
    std::atomic<int> fails;
};
static Shared *g_sh;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__,         \
                    __LINE__, #cond);                                      \
            g_sh->fails.fetch_add(1);                                      \
        }                                                                  \
    } while (0)

template <typename F> static void wait_for(F f)
{
    while (!f()) {
        sched_yield();
    }
}

static P2pDesc make_desc(uint32_t root, uint64_t seq)
{
    P2pDesc d{};
    d.seq        = seq;
    d.len        = seq * 7 + root;
    d.raw_ptr    = 0x1000 * seq;
    d.base_off   = seq;
    d.pid        = (int32_t)root;
    d.tag        = (uint16_t)(seq + 100 * root);
    d.has_tag    = 1;
    d.has_handle = 1;
    for (size_t i = 0; i < sizeof(d.handle); i++) {
        d.handle[i] = (uint8_t)(seq * 3 + i + root);
    }
    return d;
}

static void check_desc(const P2pDesc *d, uint32_t root, uint64_t seq)
{
    P2pDesc e = make_desc(root, seq);
    CHECK(d && memcmp(d, &e, sizeof(e)) == 0);
}

static void rank0(P2pMbox &mb)
{
    /* fill the ring 0->1 while rank 1 holds its acks */
    for (uint64_t s = 1; s <= kD; s++) {
        CHECK(mb.can_post(0, 1, s));
        CHECK(!mb.can_post(0, 1, s + 1)); /* in order only */
        mb.post(0, 1, make_desc(0, s));
    }
    CHECK(mb.posted(0, 1) == kD && mb.acked(0, 1) == 0);
    CHECK(!mb.can_post(0, 1, kD + 1)); /* ring full: back-pressure */
    g_sh->full.store(1);
    /* the rest wraps the ring; the status slot of s - D is read before
     * descriptor s reuses the ring slot */
    for (uint64_t s = kD + 1; s <= kN + kD; s++) {
        if (s <= kN) {
            wait_for([&] { return mb.can_post(0, 1, s); });
            CHECK(s - mb.acked(0, 1) <= kD);
        }
        int32_t st = 1;
        wait_for([&] { return mb.ack_of(0, 1, s - kD, &st); });
        CHECK(st == (s - kD == kErrSeq ? kErrSt : 0));
        if (s <= kN) {
            mb.post(0, 1, make_desc(0, s));
        }
    }
    CHECK(mb.posted(0, 1) == kN && mb.acked(0, 1) == kN);
    /* nobody used the channels into rank 0 or 1->2 */
    CHECK(mb.posted(1, 0) == 0 && mb.posted(2, 0) == 0 &&
          mb.posted(1, 2) == 0 && mb.posted(0, 2) == 0);
}

static void rank1(P2pMbox &mb)
{
    /* 2->1 runs to completion while 0->1 is stuck on my missing acks */
    for (uint64_t s = 1; s <= 2; s++) {
        wait_for([&] { return mb.peek(2, 1, s) != nullptr; });
        check_desc(mb.peek(2, 1, s), 2, s);
        CHECK(mb.can_ack(2, 1, s) && !mb.can_ack(2, 1, s + 1));
        mb.ack(2, 1, s, 0);
    }
    wait_for([&] { return g_sh->go.load() == 1; });
    CHECK(mb.posted(0, 1) == kD); /* the root could not get further */
    for (uint64_t s = 1; s <= kN; s++) {
        wait_for([&] { return mb.peek(0, 1, s) != nullptr; });
        check_desc(mb.peek(0, 1, s), 0, s);
        CHECK(mb.posted(0, 1) - (s - 1) <= kD);
        CHECK(mb.can_ack(0, 1, s));
        mb.ack(0, 1, s, s == kErrSeq ? kErrSt : 0);
    }
    CHECK(mb.peek(0, 1, kN + 1) == nullptr);
}

static void rank2(P2pMbox &mb)
{
    wait_for([&] { return g_sh->full.load() == 1; });
    for (uint64_t s = 1; s <= 2; s++) {
        CHECK(mb.can_post(2, 1, s));
        mb.post(2, 1, make_desc(2, s));
    }
    int32_t st = 1;
    wait_for([&] { return mb.ack_of(2, 1, 2, &st); });
    CHECK(st == 0);
    /* my pair finished; 0->1 has not moved */
    CHECK(mb.posted(0, 1) == kD && mb.acked(0, 1) == 0);
    g_sh->go.store(1);
}

static int child(uint32_t rank, const std::string &name)
{
    alarm(60); /* a protocol bug ends the process, not the test run */
    P2pMbox mb;
    if (rank == 0) {
        CHECK(mb.create(name, kRanks, kD) == UCC_OK);
    } else {
        ucc_status_t st;
        wait_for([&] {
            st = mb.attach(name, kRanks, kD);
            return st != UCC_INPROGRESS;
        });
        CHECK(st == UCC_OK);
        wait_for([&] { return mb.ready(); });
    }
    CHECK(mb.depth() == kD);
    if (g_sh->fails.load() == 0) {
        if (rank == 0) {
            rank0(mb);
        } else if (rank == 1) {
            rank1(mb);
        } else {
            rank2(mb);
        }
    }
    return g_sh->fails.load() ? 1 : 0;
}

int main()
{
    g_sh = (Shared *)mmap(nullptr, sizeof(Shared), PROT_READ | PROT_WRITE,
                          MAP_SHARED | MAP_ANONYMOUS, -1, 0);
    if (g_sh == MAP_FAILED) {
        perror("mmap");
        return 1;
    }
    new (g_sh) Shared{};
    CHECK(p2p_clamp_depth(8) == 8 && p2p_clamp_depth(0) == 1 &&
          p2p_clamp_depth(12) == 8 && p2p_clamp_depth(1000) == 64);
    char buf[64];
    snprintf(buf, sizeof(buf), "/uccamd-p2ptest-%d", (int)getpid());
    const std::string name = buf;
    {
        /* nobody created it yet */
        P2pMbox early;
        CHECK(early.attach(name, kRanks, kD) == UCC_INPROGRESS);
        CHECK(!early.attached() && !early.ready());
    }
    pid_t pids[kRanks];
    /* rank 0, the creator, starts last: the others poll attach() */
    for (int r = (int)kRanks - 1; r >= 0; r--) {
        pids[r] = fork();
        if (pids[r] < 0) {
            perror("fork");
            return 1;
        }
        if (pids[r] == 0) {
            _exit(child((uint32_t)r, name));
        }
    }
    int bad = 0;
    /* rank 0 owns the segment and unlinks it when it leaves: reap it
     * last so that the others never attach to a vanished name */
    for (uint32_t r = 0; r < kRanks; r++) {
        int ws = 0;
        if (waitpid(pids[r], &ws, 0) < 0 || !WIFEXITED(ws) ||
            WEXITSTATUS(ws) != 0) {
            fprintf(stderr, "rank %u failed (wait status 0x%x)\n", r, ws);
            bad = 1;
        }
    }
    if (bad || g_sh->fails.load()) {
        return 1;
    }
    printf("P2P_MBOX_OK\n");
    return 0;
}
