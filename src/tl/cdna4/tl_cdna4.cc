/* TL "cdna4": the xGMI device transport for up to 8 fully-connected
 * MI355X GPUs (one process per GPU, or the in-process multi-rank jig on a
 * single GPU).
 *
 * Reference parity: replaces tl/cuda (tl_cuda_team.c scratch+IPC exchange,
 * tl_cuda_coll.h slot protocol, *_linear.c algorithms) and the NVLS
 * allreduce (tl/cuda/kernels/allreduce_kernel.cu), re-designed for CDNA4:
 *
 *  - control plane: host POSIX-shm slot segment (slot_seg.h) with monotonic
 *    step counters — same protocol as tl/shm.
 *  - data plane: per-rank device scratch (hipMalloc, HIP-IPC exported) laid
 *    out as [slot][parity][in|out] areas; peers read each other's areas
 *    directly over xGMI from gfx950 kernels (ec_hip reduce/gather), so a
 *    staged linear collective touches all 7 links simultaneously:
 *    reduce-scatter phase + allgather phase each move S/8 per link =>
 *    aggregate bus bandwidth approaches 7 x 153 GB/s per GPU.
 *  - small messages: ONE fused kernel per rank (ec_hip::fused_allreduce)
 *    that stages, signals arrival on every peer's fine-grained flag word
 *    (system-scope atomics), spins bounded, reduces — no host round trips
 *    between ranks, single kernel-launch latency.
 *
 * Algorithms here (v1): allreduce (fused small / staged-linear large),
 * allgather(v), reduce_scatter(v), bcast, reduce. Host-memory colls and
 * everything else fall back per the score map. Opt-in: the fused kernel's
 * protocol for small allgather / reduce_scatter / alltoall / bcast / reduce
 * (FusedCollTask, fused_plan.h), for allgatherv / reduce_scatterv, and for
 * alltoallv with a vote inside the kernel (FusedA2avTask); under a knob of
 * their own, for gather / scatter (FusedCollTask) and for gatherv / scatterv
 * with the root's verdict read inside the kernel (FusedRootedVTask).
 */
#include <atomic>
#include <map>
#include <mutex>

#include <hip/hip_runtime.h>

#include "../../core/core.h"
#include "../../ec/ec_hip.h"
#include "../../topo/topo.h"
#include "../../mc/mc.h"
#include "../shm/slot_seg.h"
#include "p2p_mbox.h"
#include "ring_plan.h"
#include "fused_plan.h"
#include "zc_policy.h"

namespace ucc {
namespace {

/* fire-and-forget HIP calls (cleanup paths, stream ops whose failures
 * surface later through event queries): log-and-continue. */
static inline void hip_warn_on_err(hipError_t e, const char *what)
{
    if (e != hipSuccess) {
        ucc_warn("%s: %s", what, hipGetErrorString(e));
    }
}
#define HIPWARN(expr) hip_warn_on_err((expr), #expr)

using ec_hip::kMaxRanks;
static_assert(tl_cdna4::kZcBlocksDefault == ec_hip::kGatedBlocks,
              "zc_policy.h carries the default gated grid");
static_assert(kRingMaxRings == ec_hip::kMaxRings &&
                  kRingMaxRanks == ec_hip::kMaxRanks,
              "ring_plan.h and ec_hip.h disagree");
static_assert(kFusedMaxRanks == ec_hip::kMaxRanks &&
                  kFusedRootedHdr == ec_hip::kRootedHdrBytes,
              "fused_plan.h and ec_hip.h disagree");

/* v-coll count/displacement accessors honoring the 64-bit flags
 * (reference: ucc_coll_utils count conventions). */
static inline size_t coll_count_at(const ucc_coll_args_t &a, const void *c,
                                   uint32_t i)
{
    return (a.flags & UCC_COLL_ARGS_FLAG_COUNT_64BIT)
               ? (size_t)((const uint64_t *)c)[i]
               : (size_t)((const uint32_t *)c)[i];
}
static inline size_t coll_disp_at(const ucc_coll_args_t &a, const void *d,
                                  uint32_t i)
{
    return (a.flags & UCC_COLL_ARGS_FLAG_DISPLACEMENTS_64BIT)
               ? (size_t)((const uint64_t *)d)[i]
               : (size_t)((const uint32_t *)d)[i];
}

/* observability: zc exchanges that consumed user-registered mem_map
 * handles (honored src_memh/dst_memh) — regression hook for tests */
static std::atomic<uint64_t> g_memh_uses{0};
extern "C" uint64_t ucc_amd_cdna4_memh_uses()
{
    return g_memh_uses.load(std::memory_order_relaxed);
}

#define HIPCHK(expr)                                                         \
    do {                                                                     \
        hipError_t _e = (expr);                                              \
        if (_e != hipSuccess) {                                              \
            ucc_error("%s failed: %s", #expr, hipGetErrorString(_e));        \
            return UCC_ERR_NO_RESOURCE;                                      \
        }                                                                    \
    } while (0)

struct Cdna4Cfg {
    uint64_t spin_limit; /* device spin bound; 0 = kernel default */
    uint32_t nslots;
    uint32_t npers;     /* dedicated slots for persistent triggered
                           (graph-captured) collectives              */
    size_t   chunk;     /* staging fragment bytes                     */
    size_t   fused_max; /* msg sizes <= this take the fused kernel    */
    int      gated_blocks; /* gated kernel grid size (team constant)  */
    int      zc_stream;    /* tl_cdna4::ZcStreamKnob (ZC_STREAM)       */
    bool     ce_alltoall;  /* SDMA copy-engine alltoall data path     */
    size_t   ce_alltoall_min; /* min total msg bytes for the CE path  */
    bool     p2p;        /* device active-set bcast (p2p send/recv)      */
    uint32_t p2p_depth;  /* mailbox ring depth, power of two <= 64       */
    int      p2p_blocks; /* pull kernel grid size; 0 = size-derived      */
    bool     gated_rooted; /* gated_pipeline for full-team bcast/reduce  */
    bool     ring;       /* offer the multi-ring algorithms              */
    int      ring_nrings; /* rings to use, 0 = auto (ring_plan.h)        */
    bool     fused_colls; /* fused one-kernel ag/rs/a2a/bcast/reduce and
                             their v-forms                                */
    size_t   fused_colls_max; /* bound on the plan's scratch_bytes         */
    bool     fused_gather_scatter; /* fused one-kernel gather / scatter and
                                      their v-forms (same bound)           */
};

class Cdna4Tl;

class Cdna4TlContext final : public TlContext {
  public:
    Cdna4TlContext(Context *ctx, Tl *tl, int dev) : TlContext(ctx), tl_(tl),
                                                    dev_(dev)
    {
        HIPWARN(hipStreamCreateWithFlags(&comp_, hipStreamNonBlocking));
        HIPWARN(hipStreamCreateWithFlags(&copy_, hipStreamNonBlocking));
    }
    ~Cdna4TlContext() override
    {
        if (comp_) {
            HIPWARN(hipStreamDestroy(comp_));
        }
        if (copy_) {
            HIPWARN(hipStreamDestroy(copy_));
        }
        for (auto &s : ce_) {
            if (s) {
                HIPWARN(hipStreamDestroy(s));
            }
        }
    }
    Tl *iface() override;

    /* copy-engine streams: concurrent hipMemcpyAsync lanes so per-peer
     * SDMA transfers overlap (one stream would serialize the blits) */
    static constexpr int kNumCe = 4;
    hipStream_t ce(int i)
    {
        i &= kNumCe - 1;
        if (!ce_[i] &&
            hipStreamCreateWithFlags(&ce_[i], hipStreamNonBlocking) !=
                hipSuccess) {
            ce_[i] = nullptr;
        }
        return ce_[i];
    }

    Tl         *tl_;
    int         dev_;
    hipStream_t comp_ = nullptr, copy_ = nullptr;
    hipStream_t ce_[kNumCe] = {};
};

struct PeerRes {
    uint8_t  *scratch = nullptr;
    uint64_t *flags   = nullptr;
    bool      ipc_s = false, ipc_f = false;
};

struct ExchgBlob {
    int32_t           pid;
    int32_t           device;
    uint64_t          scratch_ptr;
    uint64_t          flags_ptr;
    hipIpcMemHandle_t sh;
    hipIpcMemHandle_t fh;
};

class Cdna4TlTeam final : public TlTeam {
  public:
    Cdna4TlTeam(TlContext *tlc, Team *team, const Cdna4Cfg &cfg)
        : TlTeam(tlc, team), cfg_(cfg)
    {
        char buf[96];
        snprintf(buf, sizeof(buf), "/uccamd-c4-%016llx-%u",
                 (unsigned long long)team->team_uid,
                 (unsigned)(team->team_uid >> 48));
        seg_name_ = buf;
        init_st_  = local_init();
        if (init_st_ == UCC_OK && team->rank == 0) {
            init_st_ = seg_.create(seg_name_, team->size, cfg_.nslots, 0);
        }
        mbox_name_ = seg_name_ + "-p2p";
        if (init_st_ == UCC_OK && cfg_.p2p && team->rank == 0) {
            init_st_ = mbox_.create(mbox_name_, team->size, cfg_.p2p_depth);
        }
        p2p_send_seq_.assign(team->size, 0);
        p2p_recv_seq_.assign(team->size, 0);
        p2p_recv_taken_.assign(team->size, 0);
        p2p_send_read_.assign(team->size, 0);
    }

    /* team-lifetime IPC import cache: user-buffer handles opened for
     * zero-copy stay mapped until the team dies, so re-created
     * persistent colls on the same tensors (e.g. a rebuilt DDP bucket)
     * skip the hipIpcOpenMemHandle on every rank (reference mem_map /
     * rcache role for the xGMI path).
     *
     * Lifecycle (reference tl_cuda_cache.c:113-140 invalidate role):
     * keyed by (exporter pid, exporter base VA). A hit re-validates the
     * HANDLE BYTES — if the exporter freed and a new allocation landed
     * on the same VA, the handle differs and the stale mapping is
     * closed and re-opened. Conversely a NEW (pid,va) whose handle
     * bytes match a cached entry at a DIFFERENT va means the driver
     * recycled the handle identity after a free: the old entry is
     * stale and must be closed BEFORE the open (an open of the same
     * handle can return the old refcounted mapping). */
    void *ipc_open_cached(int32_t pid, uint64_t remote_base,
                          const hipIpcMemHandle_t &h)
    {
        std::string hb((const char *)&h, sizeof(h));
        auto        key = std::make_pair(pid, remote_base);
        std::lock_guard<std::mutex> g(ipc_mu_);
        auto it = ipc_cache_.find(key);
        if (it != ipc_cache_.end()) {
            if (it->second.handle == hb) {
                return it->second.mapped;
            }
            HIPWARN(hipIpcCloseMemHandle(it->second.mapped));
            ipc_cache_.erase(it);
        }
        for (auto jt = ipc_cache_.begin(); jt != ipc_cache_.end();) {
            if (jt->second.handle == hb) {
                HIPWARN(hipIpcCloseMemHandle(jt->second.mapped));
                jt = ipc_cache_.erase(jt);
            } else {
                ++jt;
            }
        }
        void *m = nullptr;
        if (hipIpcOpenMemHandle(&m, h, hipIpcMemLazyEnablePeerAccess) !=
            hipSuccess) {
            return nullptr;
        }
        ipc_cache_[key] = IpcEnt{hb, m};
        return m;
    }
    struct IpcEnt {
        std::string handle;
        void       *mapped;
    };
    std::map<std::pair<int32_t, uint64_t>, IpcEnt> ipc_cache_;
    std::mutex                    ipc_mu_;

    ~Cdna4TlTeam() override
    {
        for (auto &kv : ipc_cache_) {
            HIPWARN(hipIpcCloseMemHandle(kv.second.mapped));
        }
        for (uint32_t r = 0; r < (uint32_t)peers_.size(); r++) {
            if (peers_[r].ipc_s) {
                HIPWARN(hipIpcCloseMemHandle(peers_[r].scratch));
            }
            if (peers_[r].ipc_f) {
                HIPWARN(hipIpcCloseMemHandle(peers_[r].flags));
            }
        }
        if (scratch_) {
            HIPWARN(hipFree(scratch_));
        }
        if (flags_) {
            HIPWARN(hipFree(flags_));
        }
        if (err_host_) {
            HIPWARN(hipHostFree(err_host_));
        }
        if (p2p_cnt_) {
            HIPWARN(hipFree(p2p_cnt_));
        }
    }

    ucc_status_t local_init()
    {
        /* scratch: [slot][parity][in|out] areas of chunk bytes each;
         * slots [0, nslots) rotate for host-driven colls, slots
         * [nslots, nslots+npers) are pinned to persistent triggered
         * (graph-replayable) requests */
        scratch_bytes_ =
            (size_t)(cfg_.nslots + cfg_.npers) * 2 * 2 * cfg_.chunk;
        HIPCHK(hipMalloc((void **)&scratch_, scratch_bytes_));
        pslot_used_.assign(cfg_.npers, false);
        pslot_kind_.assign(cfg_.npers, 0);
        /* flags: fine-grained for cross-GPU system-scope atomics */
        hipError_t e =
            hipExtMallocWithFlags((void **)&flags_, ec_hip::kFlagsBytes,
                                  hipDeviceMallocFinegrained);
        if (e != hipSuccess) {
            ucc_warn("finegrained alloc failed (%s), using hipMalloc",
                     hipGetErrorString(e));
            HIPCHK(hipMalloc((void **)&flags_, ec_hip::kFlagsBytes));
        }
        HIPCHK(hipMemset(flags_, 0, ec_hip::kFlagsBytes));
        HIPCHK(hipHostMalloc((void **)&err_host_, 512,
                             hipHostMallocDefault));
        memset((void *)err_host_, 0, 512);
        done_host_  = err_host_ + 8;  /* [8..15]: per-slot fused flags */
        /* [32..39]: per-slot verdict of the fused alltoallv's vote */
        verdict_host_ = err_host_ + 32;
        gdone_host_ = err_host_ + 16; /* [16..23]: per-slot gated flags */
        p2p_done_host_ = err_host_ + 24; /* [24]: p2p pull launch seq   */
        /* p2p pull arrival counter: an allocation of its own, clear of
         * the flags_ layout documented in ec_hip.h */
        HIPCHK(hipMalloc((void **)&p2p_cnt_, 64));
        HIPCHK(hipMemset(p2p_cnt_, 0, 64));
        gdone_seq_.assign(ec_hip::kGatedSlots, 0);
        HIPCHK(hipDeviceSynchronize());
        return UCC_OK;
    }

    size_t exchg_size() override { return sizeof(ExchgBlob); }

    void exchg_pack(void *buf) override
    {
        ExchgBlob b{};
        b.pid         = (int32_t)getpid();
        b.device      = ((Cdna4TlContext *)tlc_)->dev_;
        b.scratch_ptr = (uint64_t)(uintptr_t)scratch_;
        b.flags_ptr   = (uint64_t)(uintptr_t)flags_;
        if (init_st_ == UCC_OK) {
            HIPWARN(hipIpcGetMemHandle(&b.sh, scratch_));
            HIPWARN(hipIpcGetMemHandle(&b.fh, flags_));
        }
        memcpy(buf, &b, sizeof(b));
    }

    ucc_status_t exchg_unpack(const void *all, size_t stride) override
    {
        if (init_st_ != UCC_OK) {
            return init_st_;
        }
        const uint32_t n  = team_->size;
        const int32_t  me = (int32_t)getpid();
        peers_.resize(n);
        dev_map_.resize(n);
        /* Topology gate (reference tl_cuda_team_topo.c:56-100 role):
         * every pair must be xGMI/peer-access reachable or same-device,
         * or this TL refuses the team and the score fallback chain
         * (rccl, shm staging) takes over instead of hanging on an
         * unreachable IPC read. Spin bounds scale with the worst hop
         * count so remote-peer latency is not misread as a timeout. */
        {
            int mydev = ((Cdna4TlContext *)tlc_)->dev_;
            const topo::GpuLinks &gl = topo::gpu_links();
            max_hops_ = 1;
            for (uint32_t r = 0; r < n; r++) {
                ExchgBlob b;
                memcpy(&b, (const uint8_t *)all + r * stride, sizeof(b));
                dev_map_[r] = b.device;
                if (b.device == mydev || r == team_->rank) {
                    continue;
                }
                if (b.device < gl.ndev && mydev < gl.ndev &&
                    b.device >= 0) {
                    if (!gl.peer[mydev][b.device]) {
                        ucc_warn("cdna4: no peer access dev%d->dev%d "
                                 "(rank %u); dropping cdna4 team "
                                 "(fallback TLs take over)",
                                 mydev, b.device, r);
                        return UCC_ERR_NOT_SUPPORTED;
                    }
                    int h = gl.hops[mydev][b.device];
                    if (h > (int)max_hops_) {
                        max_hops_ = (uint32_t)h;
                    }
                }
            }
        }
        for (uint32_t r = 0; r < n; r++) {
            ExchgBlob b;
            memcpy(&b, (const uint8_t *)all + r * stride, sizeof(b));
            if (r == team_->rank) {
                peers_[r].scratch = scratch_;
                peers_[r].flags   = flags_;
            } else if (b.pid == me) {
                /* in-process jig: same address space */
                peers_[r].scratch = (uint8_t *)(uintptr_t)b.scratch_ptr;
                peers_[r].flags   = (uint64_t *)(uintptr_t)b.flags_ptr;
            } else {
                void *p = nullptr;
                hipError_t e = hipIpcOpenMemHandle(
                    &p, b.sh, hipIpcMemLazyEnablePeerAccess);
                if (e != hipSuccess) {
                    ucc_warn("IPC open scratch of rank %u failed: %s", r,
                             hipGetErrorString(e));
                    return UCC_ERR_NO_RESOURCE;
                }
                peers_[r].scratch = (uint8_t *)p;
                peers_[r].ipc_s   = true;
                e = hipIpcOpenMemHandle(&p, b.fh,
                                        hipIpcMemLazyEnablePeerAccess);
                if (e != hipSuccess) {
                    ucc_warn("IPC open flags of rank %u failed: %s", r,
                             hipGetErrorString(e));
                    return UCC_ERR_NO_RESOURCE;
                }
                peers_[r].flags = (uint64_t *)p;
                peers_[r].ipc_f = true;
            }
        }
        return UCC_OK;
    }

    ucc_status_t create_test() override
    {
        if (init_st_ != UCC_OK) {
            return init_st_;
        }
        if (team_->rank == 0) {
            return UCC_OK;
        }
        if (!attached_) {
            ucc_status_t st =
                seg_.attach(seg_name_, team_->size, cfg_.nslots, 0);
            if (st == UCC_INPROGRESS) {
                return UCC_INPROGRESS;
            }
            if (st != UCC_OK) {
                return st;
            }
            attached_ = true;
        }
        if (cfg_.p2p && !mbox_.attached()) {
            ucc_status_t st =
                mbox_.attach(mbox_name_, team_->size, cfg_.p2p_depth);
            if (st != UCC_OK) {
                return st; /* INPROGRESS: creator not there yet */
            }
        }
        return seg_.ready() && (!cfg_.p2p || mbox_.ready())
                   ? UCC_OK
                   : UCC_INPROGRESS;
    }

    void get_scores(Team *team, ScoreMap &map) override;

    /* What the score map's gated_pipeline and staged_linear / fused
     * allreduce entries build, with their checks. init_unfused: the task a
     * request gets with UCC_TL_CDNA4_FUSED_COLLS unset (gated where that
     * entry exists and accepts, else staged), and its algorithm name. */
    ucc_status_t init_gated(const ucc_coll_args_t &args, Team *t,
                            Task **task);
    ucc_status_t init_staged(const ucc_coll_args_t &args, Team *t,
                             bool fused, Task **task);
    ucc_status_t init_unfused(const ucc_coll_args_t &args, Team *t,
                              Task **task, const char **alg);

    uint8_t *area(uint32_t rank, uint32_t slot, uint32_t parity, int which)
    {
        return peers_[rank].scratch +
               (((size_t)slot * 2 + parity) * 2 + which) * cfg_.chunk;
    }

    /* Persistent-slot allocator. Deterministic across ranks as long as
     * persistent triggered requests are created/finalized in the same
     * order on every rank (collective semantics): lowest matching index.
     * A slot's device-side graph counters are NEVER reset, so a slot may
     * only be reused by a request with the SAME kernel pattern (kind):
     * counters then continue monotonically and stay consistent. */
    enum PslotKind { PK_NONE = 0, PK_FUSED, PK_G_AR, PK_G_RS, PK_G_AG,
                     PK_G_A2A };
    int alloc_pslot(int kind)
    {
        /* first pass: same-kind slot; second: never-used slot */
        for (uint32_t i = 0; i < cfg_.npers; i++) {
            if (!pslot_used_[i] && pslot_kind_[i] == kind) {
                pslot_used_[i] = true;
                return (int)(cfg_.nslots + i);
            }
        }
        for (uint32_t i = 0; i < cfg_.npers; i++) {
            if (!pslot_used_[i] && pslot_kind_[i] == PK_NONE) {
                pslot_used_[i] = true;
                pslot_kind_[i] = kind;
                return (int)(cfg_.nslots + i);
            }
        }
        return -1;
    }
    void free_pslot(int slot)
    {
        if (slot >= (int)cfg_.nslots) {
            pslot_used_[slot - cfg_.nslots] = false;
        }
    }
    std::vector<int> pslot_kind_;

    Cdna4Cfg    cfg_;
    ShmSeg      seg_;
    std::string seg_name_;
    std::vector<bool> pslot_used_;
    /* device-gated pipeline: cumulative kernel-launch counts per
     * (phase, slot, parity) — identical on every rank because
     * collectives post in the same order (targets = count x 32 blocks) */
    uint64_t gated_launch_[3][ec_hip::kGatedSlots][2] = {};
    std::vector<int> dev_map_;  /* rank -> hip device (topology gate) */
    uint32_t         max_hops_ = 1;
    /* spin bound scaled by the farthest peer's hop count (user
     * override wins) */
    uint64_t spin_limit() const
    {
        if (cfg_.spin_limit) {
            return cfg_.spin_limit;
        }
        return max_hops_ > 1
                   ? ec_hip::kDefaultSpinLimit * (uint64_t)max_hops_
                   : 0; /* 0 = kernel default */
    }
    uint64_t    seq_ = 0;
    std::vector<uint64_t> stage_cum_; /* per-slot fused block arrivals */
    uint8_t    *scratch_ = nullptr;
    size_t      scratch_bytes_ = 0;
    uint64_t   *flags_ = nullptr;  /* device fine-grained               */
    uint64_t   *err_host_  = nullptr; /* host-pinned, device-writable   */
    uint64_t   *done_host_ = nullptr; /* per-slot fused completion flags */
    uint64_t   *verdict_host_ = nullptr; /* per-slot fused alltoallv votes */
    uint64_t   *gdone_host_ = nullptr; /* per-slot gated completion flags */
    std::vector<uint64_t> done_cum_;  /* cumulative completion arrivals  */
    std::vector<uint64_t> gdone_seq_; /* per-slot gated completion seqs  */
    std::vector<PeerRes> peers_;
    ucc_status_t init_st_ = UCC_OK;
    bool         attached_ = false;
    /* device active-set bcast (ActiveSetBcastTask): per-pair mailbox and
     * this rank's host state of its channels, all under p2p_mu_. None of
     * it touches seq_, the slots or gated_launch_. */
    P2pMbox      mbox_;
    std::string  mbox_name_;
    std::mutex   p2p_mu_;
    std::vector<uint64_t> p2p_send_seq_;   /* [member]: last seq taken   */
    std::vector<uint64_t> p2p_recv_seq_;   /* [root]: last seq taken     */
    std::vector<uint64_t> p2p_recv_taken_; /* [root]: last seq consumed  */
    std::vector<uint64_t> p2p_send_read_;  /* [member]: last ack read    */
    uint64_t    *p2p_cnt_       = nullptr; /* device arrival counter     */
    uint64_t    *p2p_done_host_ = nullptr; /* host-pinned launch seq     */
    uint64_t     p2p_blocks_cum_ = 0;      /* blocks launched so far     */
    uint64_t     p2p_launches_   = 0;
};

/* -------------------------------------------------------------- tasks  */
class Cdna4Task : public Task {
  public:
    Cdna4Task(Context *ctx, Cdna4TlTeam *tt, const ucc_coll_args_t &args)
        : Task(ctx), tt_(tt), a_(args)
    {
    }
    ~Cdna4Task() override
    {
        for (auto ev : evs_) {
            if (ev) {
                HIPWARN(hipEventDestroy(ev));
            }
        }
    }

  protected:
    hipEvent_t ev(int i)
    {
        while ((int)evs_.size() <= i) {
            evs_.push_back(nullptr);
        }
        if (!evs_[i]) {
            HIPWARN(hipEventCreateWithFlags(&evs_[i], hipEventDisableTiming));
        }
        return evs_[i];
    }

    void publish(uint64_t k)
    {
        tt_->seg_.step(slot_, me_)->store(base_ + k,
                                          std::memory_order_release);
    }
    void close_slot()
    {
        tt_->seg_.step(slot_, me_)->store(base_ + kCap,
                                          std::memory_order_release);
    }
    bool all_ge(uint64_t k)
    {
        for (uint32_t r = 0; r < n_; r++) {
            if (tt_->seg_.step(slot_, r)->load(std::memory_order_acquire) <
                base_ + k) {
                return false;
            }
        }
        return true;
    }

    void begin_use()
    {
        me_          = tt_->team_->rank;
        n_           = tt_->team_->size;
        uint64_t use = tt_->seq_++;
        slot_        = (uint32_t)(use % tt_->cfg_.nslots);
        base_        = (use / tt_->cfg_.nslots) * kCap;
        fseq_        = use / tt_->cfg_.nslots + 1;
        phase_       = 0;
        frag_        = 0;
    }

    hipStream_t comp() { return ((Cdna4TlContext *)tt_->tlc_)->comp_; }
    hipStream_t copy_s() { return ((Cdna4TlContext *)tt_->tlc_)->copy_; }

    Cdna4TlTeam    *tt_;
    ucc_coll_args_t a_;
    std::vector<hipEvent_t> evs_;
    uint32_t me_ = 0, n_ = 1, slot_ = 0;
    uint64_t base_ = 0, fseq_ = 0;
    int      phase_ = 0;
    size_t   frag_  = 0;
};

/* Fused single-kernel allreduce (small messages). */
class FusedAllreduceTask final : public Cdna4Task {
  public:
    using Cdna4Task::Cdna4Task;

    ucc_status_t post() override
    {
        begin_use();
        bytes_ = a_.dst.info.count * ucc_dt_size(a_.dst.info.datatype);
        status = UCC_INPROGRESS;
        return progress();
    }

    ucc_status_t progress() override
    {
        if (phase_ == 0) {
            if (!all_ge(0)) {
                return UCC_INPROGRESS;
            }
            ec_hip::FusedArgs fa{};
            const bool inplace = a_.flags & UCC_COLL_ARGS_FLAG_IN_PLACE;
            fa.dst     = a_.dst.info.buffer;
            fa.src     = inplace ? fa.dst : a_.src.info.buffer;
            fa.count   = a_.dst.info.count;
            fa.dt      = a_.dst.info.datatype;
            fa.op      = a_.op == UCC_OP_AVG ? UCC_OP_SUM : a_.op;
            fa.alpha   = a_.op == UCC_OP_AVG ? 1.0 / (double)n_ : 1.0;
            if (a_.op == UCC_OP_AVG) {
                fa.op = (ucc_reduction_op_t)12; /* SUM+alpha path */
            }
            fa.my_scratch = tt_->area(me_, slot_, 0, 0);
            for (uint32_t r = 0; r < n_; r++) {
                fa.peer_scratch[r] = tt_->area(r, slot_, 0, 0);
                fa.peer_flags[r]   = tt_->peers_[r].flags;
            }
            fa.local_flags = tt_->flags_;
            fa.rank        = (int)me_;
            fa.nranks      = (int)n_;
            fa.slot        = (int)slot_;
            fa.seq         = fseq_;
            fa.error_word  = tt_->err_host_;
            fa.spin_limit  = tt_->spin_limit();
            size_t blocks  = (bytes_ + 128 * 1024 - 1) / (128 * 1024);
            fa.nblocks     = (int)(blocks < 1 ? 1 : blocks > 16 ? 16 : blocks);
            if (tt_->stage_cum_.size() < tt_->cfg_.nslots) {
                tt_->stage_cum_.assign(tt_->cfg_.nslots, 0);
                tt_->done_cum_.assign(tt_->cfg_.nslots, 0);
            }
            tt_->stage_cum_[slot_] += (uint64_t)fa.nblocks;
            fa.stage_target = tt_->stage_cum_[slot_];
            /* host-pinned completion flag instead of event
             * record+query (µs-class small-message latency saving) */
            tt_->done_cum_[slot_] += (uint64_t)fa.nblocks;
            fa.done_target = tt_->done_cum_[slot_];
            fa.done_seq    = fseq_;
            fa.done_host   = tt_->done_host_ + slot_;
            ucc_status_t st = ec_hip::fused_allreduce(fa, comp());
            if (st != UCC_OK) {
                return st;
            }
            phase_ = 1;
        }
        if (phase_ == 1) {
            if (*tt_->err_host_ != 0) {
                ucc_error("fused allreduce timed out waiting for peers");
                close_slot();
                return UCC_ERR_TIMED_OUT;
            }
            if (__atomic_load_n(tt_->done_host_ + slot_,
                                __ATOMIC_ACQUIRE) < fseq_) {
                return UCC_INPROGRESS;
            }
            close_slot();
            return UCC_OK;
        }
        return UCC_INPROGRESS;
    }

    /* Stream-triggered (and hipGraph-capturable) post: launch ONE fused
     * kernel with a device-derived iteration number onto the EE stream.
     * Completion is stream-ordered (request status = OK on return); the
     * same capture replays as a fresh collective iteration each time.
     * Requires a per-team dedicated slot (all ranks replay in lockstep).
     * Reference parity: ucc_triggered_post (core/ucc_coll.c:510-659) +
     * persistent executor-in-stream design, collapsed to one kernel. */
    ucc_status_t triggered_post(void *ee_stream) override
    {
        size_t bytes =
            a_.dst.info.count * ucc_dt_size(a_.dst.info.datatype);
        if (bytes > tt_->cfg_.chunk) {
            return UCC_ERR_NOT_SUPPORTED;
        }
        if (pslot_ < 0) {
            pslot_ = tt_->alloc_pslot(Cdna4TlTeam::PK_FUSED);
            if (pslot_ < 0) {
                ucc_error("no free persistent slot (TL_CDNA4 "
                          "PERSISTENT_SLOTS exhausted or pattern "
                          "mismatch)");
                return UCC_ERR_NO_RESOURCE;
            }
            me_ = tt_->team_->rank;
            n_  = tt_->team_->size;
        }
        ec_hip::GraphFusedArgs ga{};
        const bool inplace = a_.flags & UCC_COLL_ARGS_FLAG_IN_PLACE;
        ga.dst     = a_.dst.info.buffer;
        ga.src     = inplace ? ga.dst : a_.src.info.buffer;
        ga.count   = a_.dst.info.count;
        ga.dt      = a_.dst.info.datatype;
        ga.op      = a_.op == UCC_OP_AVG ? (ucc_reduction_op_t)12 : a_.op;
        ga.alpha   = a_.op == UCC_OP_AVG ? 1.0 / (double)n_ : 1.0;
        ga.my_scratch = tt_->area(me_, (uint32_t)pslot_, 0, 0);
        for (uint32_t r = 0; r < n_; r++) {
            ga.peer_scratch[r] = tt_->area(r, (uint32_t)pslot_, 0, 0);
            ga.peer_flags[r]   = tt_->peers_[r].flags;
        }
        ga.local_flags   = tt_->flags_;
        ga.rank          = (int)me_;
        ga.nranks        = (int)n_;
        ga.slot          = pslot_;
        ga.error_word    = tt_->err_host_;
        ga.parity_stride = 2 * tt_->cfg_.chunk;
        /* FIXED grid: per-block launch counters must advance uniformly
         * across every request that ever reuses this slot */
        ga.nblocks = 8;
        ucc_status_t st =
            ec_hip::fused_allreduce_graph(ga, (hipStream_t)ee_stream);
        if (st != UCC_OK) {
            return st;
        }
        status = UCC_OK;
        return UCC_OK;
    }

    ~FusedAllreduceTask() override
    {
        if (pslot_ >= 0) {
            tt_->free_pslot(pslot_);
        }
    }

  private:
    size_t bytes_ = 0;
    int    pslot_ = -1;
};

/* what the team, the slot and a plan decide of a fused kernel's argument:
 * scratch and flag pointers, cells, segments, the reduce segment */
static void fused_args_from_plan(Cdna4TlTeam *tt, uint32_t me, uint32_t n,
                                 uint32_t slot, const FusedPlan &pl,
                                 ec_hip::FusedCollArgs *fa)
{
    fa->my_scratch = tt->area(me, slot, 0, 0);
    for (uint32_t r = 0; r < n; r++) {
        fa->peer_scratch[r] = tt->area(r, slot, 0, 0);
        fa->peer_flags[r]   = tt->peers_[r].flags;
    }
    fa->local_flags = tt->flags_;
    fa->rank        = (int)me;
    fa->nranks      = (int)n;
    fa->slot        = (int)slot;
    fa->error_word  = tt->err_host_;
    fa->n_cells     = pl.n_cells;
    for (int k = 0; k < pl.n_cells; k++) {
        fa->c_src_off[k] = pl.cell[k].src_off;
        fa->c_sc_off[k]  = pl.cell[k].scratch_off;
        fa->c_len[k]     = pl.cell[k].len;
    }
    fa->n_segs = pl.n_segs;
    for (int k = 0; k < pl.n_segs; k++) {
        fa->g_peer[k]    = pl.seg[k].peer;
        fa->g_sc_off[k]  = pl.seg[k].scratch_off;
        fa->g_dst_off[k] = pl.seg[k].dst_off;
        fa->g_len[k]     = pl.seg[k].len;
    }
    fa->r_sc_off  = pl.red_scratch_off;
    fa->r_dst_off = pl.red_dst_off;
    fa->r_count   = pl.red_count;
}

/* Fused single-kernel allgather(v) / reduce_scatter(v) / alltoall / bcast /
 * reduce (small messages; opt-in, UCC_TL_CDNA4_FUSED_COLLS). The slot
 * sequencing, the cumulative stage and completion counters and the timeout
 * are FusedAllreduceTask's, on the same words, so the two compose on one
 * slot sequence; what is staged and read comes from fused_plan.h. */
class FusedCollTask final : public Cdna4Task {
  public:
    using Cdna4Task::Cdna4Task;

    /* what the accept / decline decision and the plan need from the
     * arguments; everything but inplace of REDUCE, GATHER and SCATTER (set
     * at the root only) is equal on every rank */
    struct Shape {
        FusedColl      coll;
        ucc_datatype_t dt;
        uint64_t       block; /* bytes: per-rank block, or the vector;
                                 v-forms: the largest block             */
        bool           inplace;
        /* v-forms: bytes per rank, dst.info_v of every rank (allgatherv;
         * reduce_scatterv reads its source packed, dsp stays 0) */
        uint64_t       cnt[kFusedMaxRanks], dsp[kFusedMaxRanks];
    };
    static bool is_v(FusedColl c)
    {
        return c == FUSED_ALLGATHERV || c == FUSED_REDUCE_SCATTERV;
    }
    static bool shape(const ucc_coll_args_t &a, uint32_t n, uint32_t me,
                      Shape *s)
    {
        bool       inplace = a.flags & UCC_COLL_ARGS_FLAG_IN_PLACE;
        const bool is_root = me == (uint32_t)a.root;
        uint64_t   count;
        switch (a.coll_type) {
        case UCC_COLL_TYPE_ALLGATHERV:
        case UCC_COLL_TYPE_REDUCE_SCATTERV: {
            const bool agv = a.coll_type == UCC_COLL_TYPE_ALLGATHERV;
            s->coll = agv ? FUSED_ALLGATHERV : FUSED_REDUCE_SCATTERV;
            s->dt   = a.dst.info_v.datatype;
            if (n > (uint32_t)kFusedMaxRanks || !ucc_dt_is_predefined(s->dt)) {
                return false;
            }
            const uint64_t es = ucc_dt_size(s->dt);
            s->block          = 0;
            s->inplace        = inplace;
            for (uint32_t r = 0; r < n; r++) {
                s->cnt[r] = coll_count_at(a, a.dst.info_v.counts, r) * es;
                s->dsp[r] =
                    agv ? coll_disp_at(a, a.dst.info_v.displacements, r) * es
                        : 0;
                s->block = s->cnt[r] > s->block ? s->cnt[r] : s->block;
            }
            return true;
        }
        case UCC_COLL_TYPE_ALLGATHER:
            s->coll = FUSED_ALLGATHER;
            s->dt   = a.dst.info.datatype;
            count   = a.dst.info.count / n;
            break;
        case UCC_COLL_TYPE_ALLTOALL:
            s->coll = FUSED_ALLTOALL;
            s->dt   = a.dst.info.datatype;
            count   = a.dst.info.count / n;
            break;
        case UCC_COLL_TYPE_REDUCE_SCATTER:
            s->coll = FUSED_REDUCE_SCATTER;
            s->dt   = a.dst.info.datatype;
            count   = inplace ? a.dst.info.count / n : a.dst.info.count;
            break;
        case UCC_COLL_TYPE_BCAST:
            s->coll = FUSED_BCAST;
            s->dt   = a.src.info.datatype;
            count   = a.src.info.count;
            break;
        case UCC_COLL_TYPE_REDUCE:
            s->coll = FUSED_REDUCE;
            s->dt   = a.src.info.datatype;
            count   = a.src.info.count;
            break;
        /* the rooted copies: each rank reads the side that is significant
         * on it, and the in-place flag counts at the root only */
        case UCC_COLL_TYPE_GATHER:
            s->coll = FUSED_GATHER;
            s->dt   = is_root ? a.dst.info.datatype : a.src.info.datatype;
            count   = is_root ? a.dst.info.count / n : a.src.info.count;
            inplace = inplace && is_root;
            break;
        case UCC_COLL_TYPE_SCATTER:
            s->coll = FUSED_SCATTER;
            s->dt   = is_root ? a.src.info.datatype : a.dst.info.datatype;
            count   = is_root ? a.src.info.count / n : a.dst.info.count;
            inplace = inplace && is_root;
            break;
        default: return false;
        }
        if (!ucc_dt_is_predefined(s->dt)) {
            return false;
        }
        s->block   = count * ucc_dt_size(s->dt);
        s->inplace = inplace;
        return true;
    }

    /* Rank-invariant by construction: counts, dtype, op, n, flags and knobs
     * only, never a pointer (alignment is the kernel's business). A
     * rank-local decline would put ranks on different algorithms. gather
     * and scatter: block, n, root and knobs only; the in-place flag, which
     * only the root sets, takes no part. */
    static bool supported(const ucc_coll_args_t &a, const Cdna4TlTeam *tt)
    {
        const uint32_t n = tt->team_->size;
        Shape          s;
        /* s.block == 0 for a v-form: every count is zero */
        if (!shape(a, n, tt->team_->rank, &s) || s.block == 0 ||
            (!is_v(s.coll) && a.root >= n) ||
            (s.coll == FUSED_ALLTOALL && s.inplace)) {
            return false;
        }
        if ((s.coll == FUSED_REDUCE_SCATTER || s.coll == FUSED_REDUCE ||
             s.coll == FUSED_REDUCE_SCATTERV) &&
            !ec_hip::op_supported(s.dt, a.op)) {
            return false;
        }
        size_t bound = tt->cfg_.fused_colls_max;
        if (bound > tt->cfg_.chunk) {
            bound = tt->cfg_.chunk; /* the parity area is one chunk */
        }
        if (is_v(s.coll)) {
            /* dst.info_v.counts is the same array on every rank */
            return fused_plan_scratch_bytes_v(s.coll, (int)n, s.cnt, 0) <=
                   bound;
        }
        return s.block <= bound &&
               fused_plan_scratch_bytes(s.coll, (int)n, s.block) <= bound;
    }

    ucc_status_t post() override
    {
        begin_use();
        status = UCC_INPROGRESS;
        return progress();
    }

    ucc_status_t progress() override
    {
        if (phase_ == 0) {
            if (!all_ge(0)) {
                return UCC_INPROGRESS;
            }
            ec_hip::FusedCollArgs fa{};
            FusedPlan             pl;
            ucc_status_t          st = fill(&fa, &pl, slot_);
            if (st != UCC_OK) {
                return st;
            }
            fa.seq        = fseq_;
            fa.spin_limit = tt_->spin_limit();
            /* one block per 128 KiB of the larger of staged and read
             * bytes */
            const uint64_t big = pl.stage_bytes > pl.read_bytes
                                     ? pl.stage_bytes
                                     : pl.read_bytes;
            const uint64_t blocks = (big + 128 * 1024 - 1) / (128 * 1024);
            fa.nblocks = (int)(blocks < 1 ? 1 : blocks > 16 ? 16 : blocks);
            if (tt_->stage_cum_.size() < tt_->cfg_.nslots) {
                tt_->stage_cum_.assign(tt_->cfg_.nslots, 0);
                tt_->done_cum_.assign(tt_->cfg_.nslots, 0);
            }
            tt_->stage_cum_[slot_] += (uint64_t)fa.nblocks;
            fa.stage_target = tt_->stage_cum_[slot_];
            tt_->done_cum_[slot_] += (uint64_t)fa.nblocks;
            fa.done_target = tt_->done_cum_[slot_];
            fa.done_seq    = fseq_;
            fa.done_host   = tt_->done_host_ + slot_;
            ucc_debug("cdna4 fused %s: host-sequenced kernel (k_fused_coll), "
                      "%d blocks, %zu scratch bytes",
                      coll_type_name(a_.coll_type), fa.nblocks,
                      (size_t)pl.scratch_bytes);
            st = ec_hip::fused_coll(fa, comp());
            if (st != UCC_OK) {
                return st;
            }
            phase_ = 1;
        }
        if (phase_ == 1) {
            if (*tt_->err_host_ != 0) {
                ucc_error("fused %s timed out waiting for peers",
                          coll_type_name(a_.coll_type));
                close_slot();
                return UCC_ERR_TIMED_OUT;
            }
            if (__atomic_load_n(tt_->done_host_ + slot_,
                                __ATOMIC_ACQUIRE) < fseq_) {
                return UCC_INPROGRESS;
            }
            close_slot();
            return UCC_OK;
        }
        return UCC_INPROGRESS;
    }

    /* Stream-triggered (and hipGraph-capturable) post, as
     * FusedAllreduceTask::triggered_post: one kernel with a device-derived
     * iteration number on a PK_FUSED persistent slot. */
    ucc_status_t triggered_post(void *ee_stream) override
    {
        if (pslot_ < 0) {
            pslot_ = tt_->alloc_pslot(Cdna4TlTeam::PK_FUSED);
            if (pslot_ < 0) {
                ucc_error("no free persistent slot (TL_CDNA4 "
                          "PERSISTENT_SLOTS exhausted or pattern "
                          "mismatch)");
                return UCC_ERR_NO_RESOURCE;
            }
            me_ = tt_->team_->rank;
            n_  = tt_->team_->size;
        }
        ec_hip::FusedCollArgs ga{};
        FusedPlan             pl;
        ucc_status_t          st = fill(&ga, &pl, (uint32_t)pslot_);
        if (st != UCC_OK) {
            return st;
        }
        ga.parity_stride = 2 * tt_->cfg_.chunk;
        /* FIXED grid: per-block launch counters must advance uniformly
         * across every request that ever reuses this slot */
        ga.nblocks = 8;
        ucc_debug("cdna4 fused %s: graph kernel (k_fused_coll_graph), "
                  "%d blocks, %zu scratch bytes",
                  coll_type_name(a_.coll_type), ga.nblocks,
                  (size_t)pl.scratch_bytes);
        st = ec_hip::fused_coll_graph(ga, (hipStream_t)ee_stream);
        if (st != UCC_OK) {
            return st;
        }
        status = UCC_OK;
        return UCC_OK;
    }

    ~FusedCollTask() override
    {
        if (pslot_ >= 0) {
            tt_->free_pslot(pslot_);
        }
    }

  private:
    /* the plan and everything of the kernel argument that does not depend
     * on how the launch is sequenced */
    ucc_status_t fill(ec_hip::FusedCollArgs *fa, FusedPlan *pl, uint32_t slot)
    {
        Shape s;
        if (!shape(a_, n_, me_, &s) ||
            !(is_v(s.coll)
                  ? fused_plan_init_v(pl, s.coll, (int)n_, (int)me_, s.cnt,
                                      s.dsp, nullptr, nullptr, 0,
                                      ucc_dt_size(s.dt), s.inplace)
                  : fused_plan_init(pl, s.coll, (int)n_, (int)me_,
                                    (int)a_.root, s.block, ucc_dt_size(s.dt),
                                    s.inplace)) ||
            pl->scratch_bytes > tt_->cfg_.chunk) {
            return UCC_ERR_NOT_SUPPORTED;
        }
        void *ubuf_dst = s.coll == FUSED_BCAST ? a_.src.info.buffer
                         : is_v(s.coll)        ? a_.dst.info_v.buffer
                                               : a_.dst.info.buffer;
        fa->dst = ubuf_dst;
        fa->src = pl->src_is_dst ? ubuf_dst : a_.src.info.buffer;
        /* gather and scatter: a side that is not significant on this rank
         * is never touched, the plan has no segment resp. no cell for it */
        if (s.coll == FUSED_GATHER || s.coll == FUSED_SCATTER) {
            if (pl->n_segs == 0) {
                fa->dst = nullptr;
            }
            if (pl->n_cells == 0) {
                fa->src = nullptr;
            }
        }
        fused_args_from_plan(tt_, me_, n_, slot, *pl, fa);
        fa->dt        = s.dt;
        fa->op        = a_.op == UCC_OP_AVG ? (ucc_reduction_op_t)12 : a_.op;
        fa->alpha     = a_.op == UCC_OP_AVG ? 1.0 / (double)n_ : 1.0;
        return UCC_OK;
    }

    int pslot_ = -1;
};

/* Fused single-kernel alltoallv (small pairs; opt-in with the same knob). A
 * rank knows its send row and its recv column only, so the accept / decline
 * decision cannot look at the counts: every request that passes supported()
 * launches k_fused_a2av, the ranks vote inside the kernel whether every pair
 * fits a cell (fused_plan.h, ec_hip.h), and all of them read the same
 * verdict. "Fits": the kernel has done the exchange. "Does not fit": no dst
 * byte was touched, the slot is closed, and the request is served, on a
 * fresh slot use, by the task it would have got with the knob unset
 * (Cdna4TlTeam::init_unfused). Slot sequencing, cumulative counters and the
 * timeout are FusedCollTask's. A captured graph cannot fall back, so a
 * triggered post goes to the inner task directly. */
class FusedA2avTask final : public Cdna4Task {
  public:
    using Cdna4Task::Cdna4Task;

    static uint64_t cell_bytes(const Cdna4TlTeam *tt)
    {
        size_t bound = tt->cfg_.fused_colls_max;
        if (bound > tt->cfg_.chunk) {
            bound = tt->cfg_.chunk;
        }
        return fused_plan_a2av_cell(bound, (int)tt->team_->size);
    }

    /* knobs, n, flags and datatypes only: never the counts */
    static bool supported(const ucc_coll_args_t &a, const Cdna4TlTeam *tt)
    {
        return a.coll_type == UCC_COLL_TYPE_ALLTOALLV &&
               tt->team_->size <= (uint32_t)kFusedMaxRanks &&
               cell_bytes(tt) >= 16 &&
               !(a.flags & UCC_COLL_ARGS_FLAG_IN_PLACE) &&
               ucc_dt_is_predefined(a.src.info_v.datatype) &&
               ucc_dt_is_predefined(a.dst.info_v.datatype);
    }

    ucc_status_t post() override
    {
        begin_use();
        status = UCC_INPROGRESS;
        return progress();
    }

    ucc_status_t progress() override
    {
        if (phase_ == 0) {
            if (!all_ge(0)) {
                return UCC_INPROGRESS;
            }
            ec_hip::FusedA2avArgs fa{};
            FusedPlan             pl;
            const uint64_t        cell = cell_bytes(tt_);
            const uint64_t sdt = ucc_dt_size(a_.src.info_v.datatype);
            const uint64_t rdt = ucc_dt_size(a_.dst.info_v.datatype);
            uint64_t       sc[kFusedMaxRanks], sd[kFusedMaxRanks],
                rc[kFusedMaxRanks], rd[kFusedMaxRanks];
            for (uint32_t r = 0; r < n_; r++) {
                sc[r] = coll_count_at(a_, a_.src.info_v.counts, r) * sdt;
                sd[r] =
                    coll_disp_at(a_, a_.src.info_v.displacements, r) * sdt;
                rc[r] = coll_count_at(a_, a_.dst.info_v.counts, r) * rdt;
                rd[r] =
                    coll_disp_at(a_, a_.dst.info_v.displacements, r) * rdt;
            }
            if (!fused_plan_init_v(&pl, FUSED_ALLTOALLV, (int)n_, (int)me_,
                                   sc, sd, rc, rd, cell, 1, false) ||
                pl.scratch_bytes > tt_->cfg_.chunk) {
                return UCC_ERR_NOT_SUPPORTED;
            }
            fa.c.dst = a_.dst.info_v.buffer;
            fa.c.src = a_.src.info_v.buffer;
            fused_args_from_plan(tt_, me_, n_, slot_, pl, &fa.c);
            fa.c.seq        = fseq_;
            fa.c.spin_limit = tt_->spin_limit();
            fa.fits_local   = pl.fits_local ? 1 : 0;
            /* one block per 128 KiB of the larger of staged and read
             * bytes; the stage counter is rank-local, so grids may differ
             * between ranks */
            const uint64_t big = pl.stage_bytes > pl.read_bytes
                                     ? pl.stage_bytes
                                     : pl.read_bytes;
            const uint64_t blocks = (big + 128 * 1024 - 1) / (128 * 1024);
            fa.c.nblocks =
                (int)(blocks < 1 ? 1 : blocks > 16 ? 16 : blocks);
            if (tt_->stage_cum_.size() < tt_->cfg_.nslots) {
                tt_->stage_cum_.assign(tt_->cfg_.nslots, 0);
                tt_->done_cum_.assign(tt_->cfg_.nslots, 0);
            }
            tt_->stage_cum_[slot_] += (uint64_t)fa.c.nblocks;
            fa.c.stage_target = tt_->stage_cum_[slot_];
            tt_->done_cum_[slot_] += (uint64_t)fa.c.nblocks;
            fa.c.done_target = tt_->done_cum_[slot_];
            fa.c.done_seq    = fseq_;
            fa.c.done_host   = tt_->done_host_ + slot_;
            fa.verdict_host  = tt_->verdict_host_ + slot_;
            cell_            = (size_t)cell;
            ucc_debug("cdna4 fused alltoallv: host-sequenced kernel "
                      "(k_fused_a2av), %d blocks, cell %zu bytes",
                      fa.c.nblocks, cell_);
            ucc_status_t st = ec_hip::fused_a2av(fa, comp());
            if (st != UCC_OK) {
                return st;
            }
            phase_ = 1;
        }
        if (phase_ == 1) {
            if (*tt_->err_host_ != 0) {
                ucc_error("fused alltoallv timed out waiting for peers");
                close_slot();
                return UCC_ERR_TIMED_OUT;
            }
            if (__atomic_load_n(tt_->done_host_ + slot_,
                                __ATOMIC_ACQUIRE) < fseq_) {
                return UCC_INPROGRESS;
            }
            /* stored before the completion word's release */
            const uint64_t verdict = __atomic_load_n(
                tt_->verdict_host_ + slot_, __ATOMIC_RELAXED);
            close_slot();
            if (verdict == 2 * fseq_ + 1) {
                return UCC_OK;
            }
            /* every rank read the same verdict: all fall back together */
            ucc_status_t st = make_inner();
            if (st != UCC_OK) {
                return st;
            }
            ucc_debug("cdna4 fused alltoallv: a pair exceeds the %zu-byte "
                      "cell, served by %s",
                      cell_, inner_alg_);
            phase_ = 2;
            return inner_->post();
        }
        if (phase_ == 2) {
            return inner_->progress();
        }
        return UCC_INPROGRESS;
    }

    ucc_status_t triggered_post(void *ee_stream) override
    {
        ucc_status_t st = make_inner();
        if (st != UCC_OK) {
            return st;
        }
        st = inner_->triggered_post(ee_stream);
        if (st == UCC_OK) {
            status = inner_->status.load();
        }
        return st;
    }

    ~FusedA2avTask() override { delete inner_; }

  private:
    /* built on first need, kept across re-posts of a persistent request */
    ucc_status_t make_inner()
    {
        if (inner_) {
            return UCC_OK;
        }
        return tt_->init_unfused(a_, tt_->team_, &inner_, &inner_alg_);
    }

    Task       *inner_     = nullptr;
    const char *inner_alg_ = "";
    size_t      cell_      = 0;
};

/* Fused single-kernel gatherv / scatterv (small blocks; opt-in,
 * UCC_TL_CDNA4_FUSED_GATHER_SCATTER). The counts are significant at the root
 * only, so the accept / decline decision cannot look at them: every request
 * that passes supported() launches k_fused_rooted_v, the root publishes in
 * its scratch header whether the request fits (gatherv: every block <= B;
 * scatterv: the sum of the 16-byte strides <= B; fused_plan.h, ec_hip.h),
 * and every rank reads that one verdict. "Fits": the kernel has done the
 * copies. "Does not fit": no dst byte was touched, the slot is closed, and
 * the request is served, on a fresh slot use, by the task it has with the
 * knob unset (Cdna4TlTeam::init_unfused). Everything else is
 * FusedA2avTask's: slot sequencing, cumulative counters, the per-slot
 * verdict word, the timeout; and a triggered post, which cannot fall back
 * once captured, goes to the inner task directly. */
class FusedRootedVTask final : public Cdna4Task {
  public:
    using Cdna4Task::Cdna4Task;

    /* B of fused_plan.h, from knobs alone */
    static uint64_t bound_bytes(const Cdna4TlTeam *tt)
    {
        size_t bound = tt->cfg_.fused_colls_max;
        if (bound > tt->cfg_.chunk) {
            bound = tt->cfg_.chunk;
        }
        return fused_plan_rooted_v_bound(bound);
    }

    /* type, n, knobs and the datatype of the side that is significant on
     * this rank: never the counts, never a pointer, never the in-place
     * flag's effect on anything but which datatype the root reads */
    static bool supported(const ucc_coll_args_t &a, const Cdna4TlTeam *tt)
    {
        const uint32_t n = tt->team_->size;
        if ((a.coll_type != UCC_COLL_TYPE_GATHERV &&
             a.coll_type != UCC_COLL_TYPE_SCATTERV) ||
            n > (uint32_t)kFusedMaxRanks || a.root >= n ||
            bound_bytes(tt) < 16) {
            return false;
        }
        const bool gv      = a.coll_type == UCC_COLL_TYPE_GATHERV;
        const bool is_root = tt->team_->rank == (uint32_t)a.root;
        const bool inplace = a.flags & UCC_COLL_ARGS_FLAG_IN_PLACE;
        if (!is_root) {
            return ucc_dt_is_predefined(gv ? a.src.info.datatype
                                           : a.dst.info.datatype);
        }
        return ucc_dt_is_predefined(gv ? a.dst.info_v.datatype
                                       : a.src.info_v.datatype) &&
               (inplace || ucc_dt_is_predefined(gv ? a.src.info.datatype
                                                   : a.dst.info.datatype));
    }

    ucc_status_t post() override
    {
        begin_use();
        status = UCC_INPROGRESS;
        return progress();
    }

    ucc_status_t progress() override
    {
        if (phase_ == 0) {
            if (!all_ge(0)) {
                return UCC_INPROGRESS;
            }
            ec_hip::FusedRootedVArgs fa{};
            FusedPlan                pl;
            fill(&fa, &pl);
            fused_args_from_plan(tt_, me_, n_, slot_, pl, &fa.c);
            fa.c.seq        = fseq_;
            fa.c.spin_limit = tt_->spin_limit();
            /* one block per 128 KiB of the larger of staged and read
             * bytes; the stage counter is rank-local, so grids may differ
             * between ranks */
            const uint64_t big = pl.stage_bytes > pl.read_bytes
                                     ? pl.stage_bytes
                                     : pl.read_bytes;
            const uint64_t blocks = (big + 128 * 1024 - 1) / (128 * 1024);
            fa.c.nblocks =
                (int)(blocks < 1 ? 1 : blocks > 16 ? 16 : blocks);
            if (tt_->stage_cum_.size() < tt_->cfg_.nslots) {
                tt_->stage_cum_.assign(tt_->cfg_.nslots, 0);
                tt_->done_cum_.assign(tt_->cfg_.nslots, 0);
            }
            tt_->stage_cum_[slot_] += (uint64_t)fa.c.nblocks;
            fa.c.stage_target = tt_->stage_cum_[slot_];
            tt_->done_cum_[slot_] += (uint64_t)fa.c.nblocks;
            fa.c.done_target = tt_->done_cum_[slot_];
            fa.c.done_seq    = fseq_;
            fa.c.done_host   = tt_->done_host_ + slot_;
            fa.verdict_host  = tt_->verdict_host_ + slot_;
            bound_           = (size_t)pl.bound;
            ucc_debug("cdna4 fused %s: host-sequenced kernel "
                      "(k_fused_rooted_v), %d blocks, bound %zu bytes",
                      coll_type_name(a_.coll_type), fa.c.nblocks, bound_);
            ucc_status_t st = ec_hip::fused_rooted_v(fa, comp());
            if (st != UCC_OK) {
                return st;
            }
            phase_ = 1;
        }
        if (phase_ == 1) {
            if (*tt_->err_host_ != 0) {
                ucc_error("fused %s timed out waiting for peers",
                          coll_type_name(a_.coll_type));
                close_slot();
                return UCC_ERR_TIMED_OUT;
            }
            if (__atomic_load_n(tt_->done_host_ + slot_,
                                __ATOMIC_ACQUIRE) < fseq_) {
                return UCC_INPROGRESS;
            }
            /* stored before the completion word's release */
            const uint64_t verdict = __atomic_load_n(
                tt_->verdict_host_ + slot_, __ATOMIC_RELAXED);
            close_slot();
            if (verdict == 2 * fseq_ + 1) {
                return UCC_OK;
            }
            /* every rank read the root's verdict: all fall back together */
            ucc_status_t st = make_inner();
            if (st != UCC_OK) {
                return st;
            }
            ucc_debug("cdna4 fused %s: the counts exceed the %zu-byte "
                      "bound, served by %s",
                      coll_type_name(a_.coll_type), bound_, inner_alg_);
            phase_ = 2;
            return inner_->post();
        }
        if (phase_ == 2) {
            return inner_->progress();
        }
        return UCC_INPROGRESS;
    }

    ucc_status_t triggered_post(void *ee_stream) override
    {
        ucc_status_t st = make_inner();
        if (st != UCC_OK) {
            return st;
        }
        st = inner_->triggered_post(ee_stream);
        if (st == UCC_OK) {
            status = inner_->status.load();
        }
        return st;
    }

    ~FusedRootedVTask() override { delete inner_; }

  private:
    /* The plan and the user buffers of my role. A request the plan cannot
     * express (at the root: every count zero) still has to take part in the
     * handshake, the other ranks cannot know: it runs an empty plan whose
     * root votes "does not fit", and the fallback serves it. */
    void fill(ec_hip::FusedRootedVArgs *fa, FusedPlan *pl)
    {
        const bool gv      = a_.coll_type == UCC_COLL_TYPE_GATHERV;
        const bool is_root = me_ == (uint32_t)a_.root;
        const bool inplace =
            is_root && (a_.flags & UCC_COLL_ARGS_FLAG_IN_PLACE);
        const uint64_t B = bound_bytes(tt_);
        uint64_t       cnt[kFusedMaxRanks] = {}, dsp[kFusedMaxRanks] = {};
        uint64_t       my_len = 0, es = 1;
        if (is_root) {
            const auto &v = gv ? a_.dst.info_v : a_.src.info_v;
            es            = ucc_dt_size(v.datatype);
            for (uint32_t r = 0; r < n_; r++) {
                cnt[r] = coll_count_at(a_, v.counts, r) * es;
                dsp[r] = coll_disp_at(a_, v.displacements, r) * es;
            }
            if (!gv && !inplace) {
                my_len = a_.dst.info.count *
                         ucc_dt_size(a_.dst.info.datatype);
            }
            fa->c.src = gv ? (inplace ? nullptr : a_.src.info.buffer)
                           : a_.src.info_v.buffer;
            fa->c.dst = gv ? a_.dst.info_v.buffer
                           : (inplace ? nullptr : a_.dst.info.buffer);
        } else {
            const auto &i = gv ? a_.src.info : a_.dst.info;
            es            = ucc_dt_size(i.datatype);
            my_len        = i.count * es;
            fa->c.src     = gv ? a_.src.info.buffer : nullptr;
            fa->c.dst     = gv ? nullptr : a_.dst.info.buffer;
        }
        if (!fused_plan_init_rooted_v(pl, gv ? FUSED_GATHERV : FUSED_SCATTERV,
                                      (int)n_, (int)me_, (int)a_.root, cnt,
                                      dsp, my_len, B, es, inplace)) {
            *pl               = FusedPlan{};
            pl->bound         = B;
            pl->scratch_bytes = kFusedRootedHdr + B;
            pl->fits_local    = false;
        }
        fa->root       = (int)a_.root;
        fa->is_scatter = gv ? 0 : 1;
        fa->fits_local = pl->fits_local ? 1 : 0;
        fa->my_len     = pl->my_len;
        fa->bound      = pl->bound;
        for (uint32_t r = 0; r < n_; r++) {
            fa->tab_off[r] = pl->tab_off[r];
            fa->tab_len[r] = pl->tab_len[r];
        }
    }

    /* built on first need, kept across re-posts of a persistent request */
    ucc_status_t make_inner()
    {
        if (inner_) {
            return UCC_OK;
        }
        return tt_->init_unfused(a_, tt_->team_, &inner_, &inner_alg_);
    }

    Task       *inner_     = nullptr;
    const char *inner_alg_ = "";
    size_t      bound_     = 0;
};

/* Staged linear collectives: allreduce / allgather(v) / reduce_scatter(v) /
 * bcast / reduce / alltoall(v) / gather(v) / scatter(v). Per fragment
 * (parity p), phases:
 *   A-issue (gated) -> A-wait (event) -> publish kA
 *   B-gate all>=kA  -> issue copy(f+1), launch compute -> B-wait -> kB
 *   [allreduce only] C-gate all>=kB -> gather -> C-wait -> kC
 * Block colls fragment with granularity `chunk`; per-peer colls (alltoall,
 * scatter) partition the staging area into n cells of `cell_` bytes and
 * fragment per-peer blocks with granularity cell_. Ranks may have different
 * nfrags (v-colls): close_slot() publishes base+kCap so early finishers
 * never stall peers' all_ge() gates (slot_seg.h protocol).               */
class StagedTask final : public Cdna4Task {
  public:
    using Cdna4Task::Cdna4Task;

    ucc_status_t post() override
    {
        begin_use();
        const bool inplace = a_.flags & UCC_COLL_ARGS_FLAG_IN_PLACE;
        ct_     = a_.coll_type;
        steps_  = ct_ == UCC_COLL_TYPE_ALLREDUCE ? 3 : 2;
        alpha_  = 1.0;
        op_     = a_.op;
        if (op_ == UCC_OP_AVG) {
            op_    = (ucc_reduction_op_t)12;
            alpha_ = 1.0 / (double)n_;
        }
        cnt_.assign(n_, 0);
        dsp_.assign(n_, 0);
        rcnt_.assign(n_, 0);
        rdsp_.assign(n_, 0);
        gran_ = tt_->cfg_.chunk;
        cell_ = (tt_->cfg_.chunk / n_) & ~(size_t)255;
        switch (ct_) {
        case UCC_COLL_TYPE_ALLREDUCE:
            dt_    = a_.dst.info.datatype;
            dtsz_  = ucc_dt_size(dt_);
            total_ = a_.dst.info.count * dtsz_;
            dbuf_  = (uint8_t *)a_.dst.info.buffer;
            sbuf_  = inplace ? dbuf_ : (const uint8_t *)a_.src.info.buffer;
            break;
        case UCC_COLL_TYPE_REDUCE:
            dt_    = a_.src.info.datatype;
            dtsz_  = ucc_dt_size(dt_);
            total_ = a_.src.info.count * dtsz_;
            dbuf_  = (uint8_t *)a_.dst.info.buffer;
            sbuf_  = (inplace && me_ == a_.root)
                         ? dbuf_
                         : (const uint8_t *)a_.src.info.buffer;
            break;
        case UCC_COLL_TYPE_BCAST:
            dt_    = a_.src.info.datatype;
            dtsz_  = ucc_dt_size(dt_);
            total_ = a_.src.info.count * dtsz_;
            dbuf_  = (uint8_t *)a_.src.info.buffer;
            sbuf_  = dbuf_;
            break;
        case UCC_COLL_TYPE_REDUCE_SCATTER: {
            dt_   = a_.dst.info.datatype;
            dtsz_ = ucc_dt_size(dt_);
            size_t out_b;
            if (inplace) {
                total_ = a_.dst.info.count * dtsz_;
                out_b  = total_ / n_;
                sbuf_  = (uint8_t *)a_.dst.info.buffer;
                dbuf_  = (uint8_t *)a_.dst.info.buffer + me_ * out_b;
            } else {
                out_b  = a_.dst.info.count * dtsz_;
                total_ = out_b * n_;
                sbuf_  = (const uint8_t *)a_.src.info.buffer;
                dbuf_  = (uint8_t *)a_.dst.info.buffer;
            }
            for (uint32_t r = 0; r < n_; r++) {
                cnt_[r] = out_b;
                dsp_[r] = (size_t)r * out_b;
            }
            break;
        }
        case UCC_COLL_TYPE_REDUCE_SCATTERV: {
            dt_   = a_.dst.info_v.datatype;
            dtsz_ = ucc_dt_size(dt_);
            size_t off = 0;
            for (uint32_t r = 0; r < n_; r++) {
                cnt_[r] = coll_count_at(a_, a_.dst.info_v.counts, r) * dtsz_;
                dsp_[r] = off;
                off += cnt_[r];
            }
            total_ = off;
            sbuf_  = inplace ? (const uint8_t *)a_.dst.info_v.buffer
                             : (const uint8_t *)a_.src.info.buffer;
            dbuf_  = inplace
                         ? (uint8_t *)a_.dst.info_v.buffer + dsp_[me_]
                         : (uint8_t *)a_.dst.info_v.buffer;
            ct_ = UCC_COLL_TYPE_REDUCE_SCATTER; /* same B compute */
            break;
        }
        case UCC_COLL_TYPE_ALLGATHER: {
            dt_          = a_.dst.info.datatype;
            dtsz_        = ucc_dt_size(dt_);
            size_t block = a_.dst.info.count * dtsz_ / n_;
            for (uint32_t r = 0; r < n_; r++) {
                cnt_[r] = block;
                dsp_[r] = (size_t)r * block;
            }
            dbuf_ = (uint8_t *)a_.dst.info.buffer;
            sbuf_ = inplace ? dbuf_ + dsp_[me_]
                            : (const uint8_t *)a_.src.info.buffer;
            total_  = block;
            break;
        }
        case UCC_COLL_TYPE_ALLGATHERV: {
            dt_   = a_.dst.info_v.datatype;
            dtsz_ = ucc_dt_size(dt_);
            size_t maxb = 0;
            for (uint32_t r = 0; r < n_; r++) {
                cnt_[r] = coll_count_at(a_, a_.dst.info_v.counts, r) * dtsz_;
                dsp_[r] =
                    coll_disp_at(a_, a_.dst.info_v.displacements, r) * dtsz_;
                maxb = cnt_[r] > maxb ? cnt_[r] : maxb;
            }
            dbuf_ = (uint8_t *)a_.dst.info_v.buffer;
            sbuf_ = inplace ? dbuf_ + dsp_[me_]
                            : (const uint8_t *)a_.src.info.buffer;
            total_ = maxb;
            ct_    = UCC_COLL_TYPE_ALLGATHER; /* same A/B machinery */
            break;
        }
        case UCC_COLL_TYPE_ALLTOALL: {
            /* in place is already refused at init (inplace_alltoall);
             * kept as a second guard for a task built another way */
            if (inplace || cell_ == 0) {
                return UCC_ERR_NOT_SUPPORTED;
            }
            dt_          = a_.dst.info.datatype;
            dtsz_        = ucc_dt_size(dt_);
            size_t block = a_.dst.info.count * dtsz_ / n_;
            for (uint32_t r = 0; r < n_; r++) {
                cnt_[r] = rcnt_[r] = block;
                dsp_[r] = rdsp_[r] = (size_t)r * block;
            }
            sbuf_  = (const uint8_t *)a_.src.info.buffer;
            dbuf_  = (uint8_t *)a_.dst.info.buffer;
            total_ = block;
            gran_  = cell_;
            break;
        }
        case UCC_COLL_TYPE_ALLTOALLV: {
            /* in place is already refused at init (inplace_alltoall);
             * kept as a second guard for a task built another way */
            if (inplace || cell_ == 0) {
                return UCC_ERR_NOT_SUPPORTED;
            }
            dt_   = a_.src.info_v.datatype;
            dtsz_ = ucc_dt_size(dt_);
            size_t rdtsz = ucc_dt_size(a_.dst.info_v.datatype);
            size_t maxb  = 0;
            for (uint32_t r = 0; r < n_; r++) {
                cnt_[r] = coll_count_at(a_, a_.src.info_v.counts, r) * dtsz_;
                dsp_[r] =
                    coll_disp_at(a_, a_.src.info_v.displacements, r) * dtsz_;
                rcnt_[r] =
                    coll_count_at(a_, a_.dst.info_v.counts, r) * rdtsz;
                rdsp_[r] =
                    coll_disp_at(a_, a_.dst.info_v.displacements, r) * rdtsz;
                maxb = cnt_[r] > maxb ? cnt_[r] : maxb;
                maxb = rcnt_[r] > maxb ? rcnt_[r] : maxb;
            }
            sbuf_  = (const uint8_t *)a_.src.info_v.buffer;
            dbuf_  = (uint8_t *)a_.dst.info_v.buffer;
            total_ = maxb;
            gran_  = cell_;
            ct_    = UCC_COLL_TYPE_ALLTOALL;
            break;
        }
        case UCC_COLL_TYPE_GATHER:
        case UCC_COLL_TYPE_GATHERV: {
            const bool is_v = ct_ == UCC_COLL_TYPE_GATHERV;
            if (me_ == a_.root) {
                dt_   = is_v ? a_.dst.info_v.datatype : a_.dst.info.datatype;
                dtsz_ = ucc_dt_size(dt_);
                size_t maxb = 0;
                if (is_v) {
                    for (uint32_t r = 0; r < n_; r++) {
                        rcnt_[r] =
                            coll_count_at(a_, a_.dst.info_v.counts, r) *
                            dtsz_;
                        rdsp_[r] =
                            coll_disp_at(a_, a_.dst.info_v.displacements,
                                         r) *
                            dtsz_;
                        maxb = rcnt_[r] > maxb ? rcnt_[r] : maxb;
                    }
                    dbuf_ = (uint8_t *)a_.dst.info_v.buffer;
                } else {
                    size_t block = a_.dst.info.count * dtsz_ / n_;
                    for (uint32_t r = 0; r < n_; r++) {
                        rcnt_[r] = block;
                        rdsp_[r] = (size_t)r * block;
                    }
                    maxb  = block;
                    dbuf_ = (uint8_t *)a_.dst.info.buffer;
                }
                sbuf_ = inplace ? dbuf_ + rdsp_[me_]
                                : (const uint8_t *)a_.src.info.buffer;
                total_ = maxb;
            } else {
                dt_    = a_.src.info.datatype;
                dtsz_  = ucc_dt_size(dt_);
                sbuf_  = (const uint8_t *)a_.src.info.buffer;
                dbuf_  = nullptr;
                total_ = a_.src.info.count * dtsz_;
                cnt_[me_] = total_;
            }
            ct_ = UCC_COLL_TYPE_GATHER;
            break;
        }
        case UCC_COLL_TYPE_SCATTER:
        case UCC_COLL_TYPE_SCATTERV: {
            const bool is_v = ct_ == UCC_COLL_TYPE_SCATTERV;
            if (cell_ == 0) {
                return UCC_ERR_NOT_SUPPORTED;
            }
            if (me_ == a_.root) {
                dt_   = is_v ? a_.src.info_v.datatype : a_.src.info.datatype;
                dtsz_ = ucc_dt_size(dt_);
                size_t maxb = 0;
                if (is_v) {
                    for (uint32_t r = 0; r < n_; r++) {
                        cnt_[r] =
                            coll_count_at(a_, a_.src.info_v.counts, r) *
                            dtsz_;
                        dsp_[r] =
                            coll_disp_at(a_, a_.src.info_v.displacements,
                                         r) *
                            dtsz_;
                        maxb = cnt_[r] > maxb ? cnt_[r] : maxb;
                    }
                    sbuf_ = (const uint8_t *)a_.src.info_v.buffer;
                } else {
                    size_t block = a_.src.info.count * dtsz_ / n_;
                    for (uint32_t r = 0; r < n_; r++) {
                        cnt_[r] = block;
                        dsp_[r] = (size_t)r * block;
                    }
                    maxb  = block;
                    sbuf_ = (const uint8_t *)a_.src.info.buffer;
                }
                dbuf_ = inplace ? nullptr : (uint8_t *)a_.dst.info.buffer;
                rcnt_[me_] = inplace ? 0 : cnt_[me_];
                rdsp_[me_] = 0;
                total_     = maxb;
            } else {
                dt_    = a_.dst.info.datatype;
                dtsz_  = ucc_dt_size(dt_);
                dbuf_  = (uint8_t *)a_.dst.info.buffer;
                sbuf_  = nullptr;
                total_ = a_.dst.info.count * dtsz_;
                rcnt_[a_.root] = total_;
            }
            gran_ = cell_;
            ct_   = UCC_COLL_TYPE_SCATTER;
            break;
        }
        default: return UCC_ERR_NOT_SUPPORTED;
        }
        nfrags_ = (total_ + gran_ - 1) / gran_;
        if (nfrags_ == 0) {
            nfrags_ = 1;
        }
        status = UCC_INPROGRESS;
        return progress();
    }

    ucc_status_t progress() override
    {
        while (frag_ < nfrags_) {
            const size_t   f   = frag_;
            const uint32_t p   = (uint32_t)(f & 1);
            const uint64_t kA  = steps_ * f + 1;
            const uint64_t kB  = steps_ * f + 2;
            const uint64_t kC  = steps_ * f + 3;
            const size_t   off = f * gran_;
            const size_t   len =
                total_ - off < gran_ ? total_ - off : gran_;
            switch (phase_) {
            case 0: /* entry: first copy */
                if (!all_ge(0)) {
                    return UCC_INPROGRESS;
                }
                issue_copy(0);
                phase_ = 1;
                break;
            case 1: { /* A-wait */
                if (copy_pending_) {
                    hipError_t e = hipEventQuery(ev(0 + (int)p));
                    if (e == hipErrorNotReady) {
                        return UCC_INPROGRESS;
                    }
                    if (e != hipSuccess) {
                        return UCC_ERR_NO_RESOURCE;
                    }
                }
                publish(kA);
                phase_ = 2;
                break;
            }
            case 2: { /* B-gate */
                if (!all_ge(kA)) {
                    return UCC_INPROGRESS;
                }
                if (f + 1 < nfrags_) {
                    issue_copy(f + 1);
                }
                bool launched = launch_compute(f, p, off, len);
                if (launched) {
                    HIPWARN(hipEventRecord(ev(2), comp()));
                }
                b_launched_ = launched;
                phase_      = 3;
                break;
            }
            case 3: { /* B-wait */
                if (b_launched_) {
                    hipError_t e = hipEventQuery(ev(2));
                    if (e == hipErrorNotReady) {
                        return UCC_INPROGRESS;
                    }
                    if (e != hipSuccess) {
                        return UCC_ERR_NO_RESOURCE;
                    }
                }
                publish(kB);
                if (steps_ == 2) {
                    phase_ = 1;
                    frag_++;
                    break;
                }
                phase_ = 4;
                break;
            }
            case 4: { /* C-gate (allreduce gather) */
                if (!all_ge(kB)) {
                    return UCC_INPROGRESS;
                }
                launch_gather(f, p, off, len);
                HIPWARN(hipEventRecord(ev(3), comp()));
                phase_ = 5;
                break;
            }
            case 5: { /* C-wait */
                hipError_t e = hipEventQuery(ev(3));
                if (e == hipErrorNotReady) {
                    return UCC_INPROGRESS;
                }
                if (e != hipSuccess) {
                    return UCC_ERR_NO_RESOURCE;
                }
                publish(kC);
                phase_ = 1;
                frag_++;
                break;
            }
            }
        }
        close_slot();
        return UCC_OK;
    }

  private:
    /* stage my contribution of fragment f into in[slot][f%2] */
    void issue_copy(size_t f)
    {
        const uint32_t p   = (uint32_t)(f & 1);
        const size_t   off = f * gran_;
        size_t         len = 0;
        const uint8_t *src = nullptr;
        copy_pending_ = false;
        switch (ct_) {
        case UCC_COLL_TYPE_ALLTOALL: {
            /* per-dest cells: in[r*cell_] <- sbuf[dsp_[r]+off ..] */
            ec_hip::GatherArgs ga{};
            ga.dst_base = tt_->area(me_, slot_, p, 0);
            int k       = 0;
            for (uint32_t r = 0; r < n_; r++) {
                if (off >= cnt_[r]) {
                    continue;
                }
                size_t l = cnt_[r] - off < cell_ ? cnt_[r] - off : cell_;
                ga.srcs[k] = sbuf_ + dsp_[r] + off;
                ga.offs[k] = (uint64_t)r * cell_;
                ga.lens[k] = l;
                k++;
            }
            if (k > 0) {
                ga.n = k;
                ec_hip::gather_copy(ga, copy_s());
                copy_pending_ = true;
            }
            HIPWARN(hipEventRecord(ev(0 + (int)p), copy_s()));
            return;
        }
        case UCC_COLL_TYPE_SCATTER: {
            if (me_ == a_.root) {
                ec_hip::GatherArgs ga{};
                ga.dst_base = tt_->area(me_, slot_, p, 0);
                int k       = 0;
                for (uint32_t r = 0; r < n_; r++) {
                    if (r == me_ || off >= cnt_[r]) {
                        continue;
                    }
                    size_t l = cnt_[r] - off < cell_ ? cnt_[r] - off
                                                     : cell_;
                    ga.srcs[k] = sbuf_ + dsp_[r] + off;
                    ga.offs[k] = (uint64_t)r * cell_;
                    ga.lens[k] = l;
                    k++;
                }
                if (k > 0) {
                    ga.n = k;
                    ec_hip::gather_copy(ga, copy_s());
                    copy_pending_ = true;
                }
            }
            HIPWARN(hipEventRecord(ev(0 + (int)p), copy_s()));
            return;
        }
        case UCC_COLL_TYPE_ALLGATHER:
        case UCC_COLL_TYPE_GATHER:
            if (off < cnt_[me_]) {
                len = cnt_[me_] - off < gran_ ? cnt_[me_] - off : gran_;
                src = sbuf_ + off;
            }
            break;
        case UCC_COLL_TYPE_BCAST:
            if (me_ == a_.root && off < total_) {
                len = total_ - off < gran_ ? total_ - off : gran_;
                src = sbuf_ + off;
            }
            break;
        default:
            if (off < total_) {
                len = total_ - off < gran_ ? total_ - off : gran_;
                src = sbuf_ + off;
            }
            break;
        }
        copy_pending_ = len > 0;
        if (len > 0) {
            /* stage with a COPY KERNEL by default: kernel writes are
             * L2-coherent with the peer processes' reader kernels on
             * this device by construction, while hipMemcpyAsync may
             * ride an SDMA engine (one unreproduced data-mismatch on
             * this path is on record — NEXT_STEPS.md). SDMA staging
             * stays available via UCC_TL_CDNA4_STAGE_SDMA=1. */
            static const bool sdma = Config::instance().get_bool(
                "TL_CDNA4", "STAGE_SDMA", false);
            if (sdma) {
                HIPWARN(hipMemcpyAsync(tt_->area(me_, slot_, p, 0), src,
                                       len, hipMemcpyDeviceToDevice,
                                       copy_s()));
            } else {
                ec_hip::GatherArgs ga{};
                ga.dst_base = tt_->area(me_, slot_, p, 0);
                ga.srcs[0]  = src;
                ga.offs[0]  = 0;
                ga.lens[0]  = len;
                ga.n        = 1;
                ec_hip::gather_copy(ga, copy_s());
            }
        }
        HIPWARN(hipEventRecord(ev(0 + (int)p), copy_s()));
    }

    /* B compute for fragment f; returns whether a kernel was launched */
    bool launch_compute(size_t f, uint32_t p, size_t off, size_t len)
    {
        switch (ct_) {
        case UCC_COLL_TYPE_ALLREDUCE: {
            /* reduce my 1/n slice of the fragment into out area */
            size_t nelem = len / dtsz_;
            size_t gran  = 256 / dtsz_;
            size_t per   = (nelem / n_) / gran * gran;
            size_t b     = me_ * per;
            size_t e     = me_ == n_ - 1 ? nelem : b + per;
            if (e <= b) {
                return false;
            }
            ec_hip::ReduceArgs ra{};
            ra.dst    = tt_->area(me_, slot_, p, 1);
            ra.n_srcs = (int)n_;
            ra.count  = e - b;
            ra.dt     = dt_;
            ra.op     = op_;
            ra.alpha  = alpha_;
            for (uint32_t r = 0; r < n_; r++) {
                ra.srcs[r] = tt_->area(r, slot_, p, 0) + b * dtsz_;
            }
            ec_hip::reduce(ra, comp());
            return true;
        }
        case UCC_COLL_TYPE_REDUCE: {
            if (me_ != a_.root) {
                return false;
            }
            ec_hip::ReduceArgs ra{};
            ra.dst    = dbuf_ + off;
            ra.n_srcs = (int)n_;
            ra.count  = len / dtsz_;
            ra.dt     = dt_;
            ra.op     = op_;
            ra.alpha  = alpha_;
            for (uint32_t r = 0; r < n_; r++) {
                ra.srcs[r] = tt_->area(r, slot_, p, 0);
            }
            ec_hip::reduce(ra, comp());
            return true;
        }
        case UCC_COLL_TYPE_REDUCE_SCATTER: {
            /* my dst slice ∩ fragment */
            size_t s0 = dsp_[me_], s1 = dsp_[me_] + cnt_[me_];
            size_t f0 = off, f1 = off + len;
            size_t b  = s0 > f0 ? s0 : f0;
            size_t e  = s1 < f1 ? s1 : f1;
            if (e <= b) {
                return false;
            }
            ec_hip::ReduceArgs ra{};
            ra.dst    = dbuf_ + (b - s0);
            ra.n_srcs = (int)n_;
            ra.count  = (e - b) / dtsz_;
            ra.dt     = dt_;
            ra.op     = op_;
            ra.alpha  = alpha_;
            for (uint32_t r = 0; r < n_; r++) {
                ra.srcs[r] = tt_->area(r, slot_, p, 0) + (b - off);
            }
            ec_hip::reduce(ra, comp());
            return true;
        }
        case UCC_COLL_TYPE_ALLGATHER: {
            ec_hip::GatherArgs ga{};
            int k = 0;
            for (uint32_t r = 0; r < n_; r++) {
                if (off >= cnt_[r]) {
                    continue;
                }
                size_t l = cnt_[r] - off < tt_->cfg_.chunk
                               ? cnt_[r] - off
                               : tt_->cfg_.chunk;
                if (r == me_ && (a_.flags & UCC_COLL_ARGS_FLAG_IN_PLACE)) {
                    continue;
                }
                ga.srcs[k] = tt_->area(r, slot_, p, 0);
                ga.offs[k] = dsp_[r] + off;
                ga.lens[k] = l;
                k++;
            }
            if (k == 0) {
                return false;
            }
            ga.dst_base = dbuf_;
            ga.n        = k;
            ec_hip::gather_copy(ga, comp());
            return true;
        }
        case UCC_COLL_TYPE_BCAST: {
            if (me_ == a_.root) {
                return false;
            }
            ec_hip::GatherArgs ga{};
            ga.dst_base = dbuf_;
            ga.srcs[0]  = tt_->area((uint32_t)a_.root, slot_, p, 0);
            ga.offs[0]  = off;
            ga.lens[0]  = len;
            ga.n        = 1;
            ec_hip::gather_copy(ga, comp());
            return true;
        }
        case UCC_COLL_TYPE_ALLTOALL: {
            /* read my cell from every peer's staged fragment */
            ec_hip::GatherArgs ga{};
            ga.dst_base = dbuf_;
            int k       = 0;
            for (uint32_t r = 0; r < n_; r++) {
                if (off >= rcnt_[r]) {
                    continue;
                }
                size_t l = rcnt_[r] - off < cell_ ? rcnt_[r] - off : cell_;
                ga.srcs[k] = tt_->area(r, slot_, p, 0) + me_ * cell_;
                ga.offs[k] = rdsp_[r] + off;
                ga.lens[k] = l;
                k++;
            }
            if (k == 0) {
                return false;
            }
            ga.n = k;
            ec_hip::gather_copy(ga, comp());
            return true;
        }
        case UCC_COLL_TYPE_GATHER: {
            if (me_ != a_.root) {
                return false;
            }
            ec_hip::GatherArgs ga{};
            ga.dst_base = dbuf_;
            int k       = 0;
            for (uint32_t r = 0; r < n_; r++) {
                if (off >= rcnt_[r]) {
                    continue;
                }
                size_t l = rcnt_[r] - off < gran_ ? rcnt_[r] - off : gran_;
                if (r == me_) {
                    if (a_.flags & UCC_COLL_ARGS_FLAG_IN_PLACE) {
                        continue; /* already in place */
                    }
                    ga.srcs[k] = sbuf_ + off;
                } else {
                    ga.srcs[k] = tt_->area(r, slot_, p, 0);
                }
                ga.offs[k] = rdsp_[r] + off;
                ga.lens[k] = l;
                k++;
            }
            if (k == 0) {
                return false;
            }
            ga.n = k;
            ec_hip::gather_copy(ga, comp());
            return true;
        }
        case UCC_COLL_TYPE_SCATTER: {
            if (me_ == a_.root) {
                /* my own block: direct local copy (skipped if inplace) */
                if (!dbuf_ || off >= cnt_[me_]) {
                    return false;
                }
                size_t l = cnt_[me_] - off < cell_ ? cnt_[me_] - off
                                                   : cell_;
                ec_hip::GatherArgs ga{};
                ga.dst_base = dbuf_;
                ga.srcs[0]  = sbuf_ + dsp_[me_] + off;
                ga.offs[0]  = off;
                ga.lens[0]  = l;
                ga.n        = 1;
                ec_hip::gather_copy(ga, comp());
                return true;
            }
            if (off >= rcnt_[a_.root]) {
                return false;
            }
            size_t l = rcnt_[a_.root] - off < cell_ ? rcnt_[a_.root] - off
                                                    : cell_;
            ec_hip::GatherArgs ga{};
            ga.dst_base = dbuf_;
            ga.srcs[0] =
                tt_->area((uint32_t)a_.root, slot_, p, 0) + me_ * cell_;
            ga.offs[0] = off;
            ga.lens[0] = l;
            ga.n       = 1;
            ec_hip::gather_copy(ga, comp());
            return true;
        }
        default: return false;
        }
    }

    /* allreduce stage C: gather every rank's reduced slice */
    void launch_gather(size_t f, uint32_t p, size_t off, size_t len)
    {
        (void)f;
        size_t nelem = len / dtsz_;
        size_t gran  = 256 / dtsz_;
        size_t per   = (nelem / n_) / gran * gran;
        ec_hip::GatherArgs ga{};
        ga.dst_base = dbuf_ + off;
        int k       = 0;
        for (uint32_t r = 0; r < n_; r++) {
            size_t b = r * per;
            size_t e = r == n_ - 1 ? nelem : b + per;
            if (e <= b) {
                continue;
            }
            ga.srcs[k] = tt_->area(r, slot_, p, 1);
            ga.offs[k] = b * dtsz_;
            ga.lens[k] = (e - b) * dtsz_;
            k++;
        }
        ga.n = k;
        ec_hip::gather_copy(ga, comp());
    }

    ucc_coll_type_t ct_ = UCC_COLL_TYPE_ALLREDUCE;
    const uint8_t  *sbuf_ = nullptr;
    uint8_t        *dbuf_ = nullptr;
    ucc_datatype_t  dt_   = UCC_DT_INT8;
    size_t          dtsz_ = 1;
    ucc_reduction_op_t op_ = UCC_OP_SUM;
    double          alpha_ = 1.0;
    size_t          total_ = 0, nfrags_ = 0;
    size_t          gran_ = 0, cell_ = 0;
    std::vector<size_t> cnt_, dsp_, rcnt_, rdsp_;
    int             steps_ = 3;
    bool            copy_pending_ = false, b_launched_ = false;
};

/* Device-gated staged allreduce: the large-message fast path. All
 * fragments' stage/reduce/gather kernels are enqueued up front (stage on
 * the copy stream, reduce+gather on the compute stream); cross-rank and
 * cross-fragment ordering is enforced INSIDE the kernels by prologue
 * spins on cumulative per-(slot,parity,phase) block counters in the
 * peers' fine-grained flag buffers (ec_hip::GatedArgs) — zero host
 * round-trips inside the collective, one trailing event. Same xGMI
 * traffic as the host-gated staged path (1.75 x S per rank), minus all
 * host gating latency. */
class GatedCollTask final : public Cdna4Task {
  public:
    using Cdna4Task::Cdna4Task;

    ucc_status_t post() override
    {
        begin_use();
        if (slot_ >= (uint32_t)ec_hip::kGatedSlots) {
            return UCC_ERR_NOT_SUPPORTED;
        }
        ucc_status_t st = setup_coll();
        if (st != UCC_OK) {
            return st;
        }
        if (!zc_ready_ &&
            (ct_ == UCC_COLL_TYPE_ALLREDUCE ||
             ct_ == UCC_COLL_TYPE_REDUCE_SCATTER ||
             ct_ == UCC_COLL_TYPE_ALLGATHER ||
             ct_ == UCC_COLL_TYPE_ALLTOALL ||
             ct_ == UCC_COLL_TYPE_BCAST ||
             ct_ == UCC_COLL_TYPE_REDUCE) &&
            Config::instance().get_bool("TL_CDNA4", "ZCOPY", true)) {
            if (a_.flags & UCC_COLL_ARGS_FLAG_PERSISTENT) {
                zc_ = true; /* exchange amortized over re-posts */
            } else if (a_.flags & UCC_COLL_ARGS_FLAG_MEM_MAPPED_BUFFERS) {
                /* caller promises src/dst sit inside ucc_mem_map'd
                 * regions: imports come from the memh/IPC caches, so
                 * zero-copy pays at any size (reference MEM_MAPPED
                 * flag role, ucc.h onesided semantics) */
                zc_ = true;
            } else {
                /* one-shot: the 4 host-gated exchange rounds (team
                 * IPC-import cache makes the opens free after first
                 * contact) pay off once the staging copy they remove
                 * is big enough */
                size_t min_b = Config::instance().get_size(
                    "TL_CDNA4", "ZCOPY_ONESHOT_MIN", 16 * 1024 * 1024);
                if (min_b > 0 && total_ >= min_b) {
                    zc_ = true;
                }
            }
        }
        phase_ = zc_ && !zc_ready_ ? 10 : 0;
        if (ct_ == UCC_COLL_TYPE_ALLTOALLV && !a2av_ready_) {
            phase_ = 20; /* global-max exchange first */
        }
        status = UCC_INPROGRESS;
        return progress();
    }

    /* Stream-triggered / hipGraph-capturable post: kernels derive their
     * iteration on device (GatedArgs.derive) on a DEDICATED slot, so one
     * capture replays as a fresh collective each time — the large-message
     * counterpart of the fused graph kernel (docs/GATED_PIPELINE.md). */
    ucc_status_t triggered_post(void *ee_stream) override
    {
        if (a_.coll_type == UCC_COLL_TYPE_ALLTOALLV) {
            /* needs a host-side global-max exchange before enqueue:
             * not expressible as a pure stream capture */
            return UCC_ERR_NOT_SUPPORTED;
        }
        if (pslot_ < 0) {
            ucc_coll_type_t k_ct = a_.coll_type;
            /* bcast and reduce always run the staged allreduce launch
             * pattern here (three kernels of B blocks per iteration) */
            int kind = (k_ct == UCC_COLL_TYPE_ALLREDUCE ||
                        k_ct == UCC_COLL_TYPE_BCAST ||
                        k_ct == UCC_COLL_TYPE_REDUCE)
                           ? Cdna4TlTeam::PK_G_AR
                       : (k_ct == UCC_COLL_TYPE_REDUCE_SCATTER ||
                          k_ct == UCC_COLL_TYPE_REDUCE_SCATTERV)
                           ? Cdna4TlTeam::PK_G_RS
                       : (k_ct == UCC_COLL_TYPE_ALLGATHER ||
                          k_ct == UCC_COLL_TYPE_ALLGATHERV)
                           ? Cdna4TlTeam::PK_G_AG
                           : Cdna4TlTeam::PK_G_A2A;
            pslot_ = tt_->alloc_pslot(kind);
            if (pslot_ < 0 || pslot_ >= ec_hip::kGatedSlots) {
                ucc_error("no persistent slot for triggered gated coll "
                          "(PERSISTENT_SLOTS exhausted or pattern "
                          "mismatch)");
                return UCC_ERR_NO_RESOURCE;
            }
            me_ = tt_->team_->rank;
            n_  = tt_->team_->size;
            ucc_status_t st = setup_coll();
            if (st != UCC_OK) {
                return st;
            }
        }
        slot_ = (uint32_t)pslot_;
        ucc_status_t st = enqueue_frags((hipStream_t)ee_stream,
                                        (hipStream_t)ee_stream, true);
        if (st != UCC_OK) {
            return st;
        }
        status = UCC_OK; /* stream-ordered completion */
        return UCC_OK;
    }

  private:
    ucc_status_t setup_coll()
    {
        const bool inplace = a_.flags & UCC_COLL_ARGS_FLAG_IN_PLACE;
        ct_     = a_.coll_type;
        op_     = a_.op;
        alpha_  = 1.0;
        gran_   = tt_->cfg_.chunk;
        cell_   = (tt_->cfg_.chunk / n_) & ~(size_t)255;
        if (op_ == UCC_OP_AVG) {
            op_    = (ucc_reduction_op_t)12;
            alpha_ = 1.0 / (double)n_;
        }
        switch (ct_) {
        case UCC_COLL_TYPE_ALLREDUCE:
            dt_    = a_.dst.info.datatype;
            dtsz_  = ucc_dt_size(dt_);
            total_ = a_.dst.info.count * dtsz_;
            dbuf_  = (uint8_t *)a_.dst.info.buffer;
            sbuf_  = inplace ? dbuf_ : (const uint8_t *)a_.src.info.buffer;
            break;
        case UCC_COLL_TYPE_BCAST:
            /* fragments and slices of allreduce; one buffer is source
             * (root) and destination (everyone else) */
            if (a_.root >= n_) {
                return UCC_ERR_INVALID_PARAM;
            }
            dt_    = a_.src.info.datatype;
            dtsz_  = ucc_dt_size(dt_);
            total_ = a_.src.info.count * dtsz_;
            dbuf_  = (uint8_t *)a_.src.info.buffer;
            sbuf_  = dbuf_;
            break;
        case UCC_COLL_TYPE_REDUCE:
            /* dst.info is valid at the root only. A non-root rank has no
             * destination: dbuf_ stays null there and no launch is ever
             * handed it (empty gather slices; zero-copy writes go to the
             * ROOT's mapped dst). */
            if (a_.root >= n_) {
                return UCC_ERR_INVALID_PARAM;
            }
            dt_    = a_.src.info.datatype;
            dtsz_  = ucc_dt_size(dt_);
            total_ = a_.src.info.count * dtsz_;
            if (me_ == (uint32_t)a_.root) {
                dbuf_ = (uint8_t *)a_.dst.info.buffer;
                sbuf_ = inplace ? dbuf_
                                : (const uint8_t *)a_.src.info.buffer;
            } else {
                dbuf_ = nullptr;
                sbuf_ = (const uint8_t *)a_.src.info.buffer;
            }
            break;
        case UCC_COLL_TYPE_REDUCE_SCATTER: {
            dt_   = a_.dst.info.datatype;
            dtsz_ = ucc_dt_size(dt_);
            size_t out_b;
            if (inplace) {
                total_ = a_.dst.info.count * dtsz_;
                out_b  = total_ / n_;
                sbuf_  = (uint8_t *)a_.dst.info.buffer;
                dbuf_  = (uint8_t *)a_.dst.info.buffer + me_ * out_b;
            } else {
                out_b  = a_.dst.info.count * dtsz_;
                total_ = out_b * n_;
                sbuf_  = (const uint8_t *)a_.src.info.buffer;
                dbuf_  = (uint8_t *)a_.dst.info.buffer;
            }
            out_b_ = out_b;
            break;
        }
        case UCC_COLL_TYPE_ALLGATHER: {
            dt_    = a_.dst.info.datatype;
            dtsz_  = ucc_dt_size(dt_);
            size_t block = a_.dst.info.count * dtsz_ / n_;
            out_b_ = block;
            cnt_.assign(n_, block);
            dsp_.resize(n_);
            for (uint32_t r = 0; r < n_; r++) {
                dsp_[r] = (size_t)r * block;
            }
            dbuf_  = (uint8_t *)a_.dst.info.buffer;
            sbuf_  = inplace ? dbuf_ + me_ * block
                             : (const uint8_t *)a_.src.info.buffer;
            total_ = block; /* fragment over the per-rank block */
            break;
        }
        case UCC_COLL_TYPE_ALLGATHERV: {
            /* per-rank counts are global knowledge (dst.info_v), so the
             * symmetric-launch invariant holds: every rank launches
             * ceil(max_block / chunk) fragments (empty tails still
             * launch and signal) */
            dt_   = a_.dst.info_v.datatype;
            dtsz_ = ucc_dt_size(dt_);
            cnt_.resize(n_);
            dsp_.resize(n_);
            size_t maxb = 0;
            for (uint32_t r = 0; r < n_; r++) {
                cnt_[r] = coll_count_at(a_, a_.dst.info_v.counts, r) *
                          dtsz_;
                dsp_[r] =
                    coll_disp_at(a_, a_.dst.info_v.displacements, r) *
                    dtsz_;
                maxb = cnt_[r] > maxb ? cnt_[r] : maxb;
            }
            dbuf_  = (uint8_t *)a_.dst.info_v.buffer;
            sbuf_  = inplace ? dbuf_ + dsp_[me_]
                             : (const uint8_t *)a_.src.info.buffer;
            total_ = maxb;
            ct_    = UCC_COLL_TYPE_ALLGATHERV;
            break;
        }
        case UCC_COLL_TYPE_REDUCE_SCATTERV: {
            dt_   = a_.dst.info_v.datatype;
            dtsz_ = ucc_dt_size(dt_);
            cnt_.resize(n_);
            dsp_.resize(n_);
            size_t off = 0;
            for (uint32_t r = 0; r < n_; r++) {
                cnt_[r] = coll_count_at(a_, a_.dst.info_v.counts, r) *
                          dtsz_;
                dsp_[r] = off;
                off += cnt_[r];
            }
            total_ = off;
            sbuf_  = inplace ? (const uint8_t *)a_.dst.info_v.buffer
                             : (const uint8_t *)a_.src.info.buffer;
            dbuf_  = inplace
                         ? (uint8_t *)a_.dst.info_v.buffer + dsp_[me_]
                         : (uint8_t *)a_.dst.info_v.buffer;
            ct_ = UCC_COLL_TYPE_REDUCE_SCATTERV;
            break;
        }
        case UCC_COLL_TYPE_ALLTOALL: {
            /* in place is already refused at init (inplace_alltoall);
             * kept as a second guard for a task built another way */
            if (inplace || cell_ == 0) {
                return UCC_ERR_NOT_SUPPORTED;
            }
            dt_    = a_.dst.info.datatype;
            dtsz_  = ucc_dt_size(dt_);
            out_b_ = a_.dst.info.count * dtsz_ / n_; /* per-peer block */
            sbuf_  = (const uint8_t *)a_.src.info.buffer;
            dbuf_  = (uint8_t *)a_.dst.info.buffer;
            total_ = out_b_;
            gran_  = cell_;
            break;
        }
        case UCC_COLL_TYPE_ALLTOALLV: {
            /* Per-peer send row (src.info_v) and recv column
             * (dst.info_v) are LOCAL knowledge, but the symmetric-launch
             * invariant needs the GLOBAL max pair length — exchanged
             * host-side through the scratch channel (phases 20/21)
             * before any fragment is enqueued. Rank i's send cell to j
             * and its gather of j's cell both clip to the locally-known
             * lengths; empty tails still launch and signal. */
            /* in place is already refused at init (inplace_alltoall);
             * kept as a second guard for a task built another way */
            if (inplace || cell_ == 0) {
                return UCC_ERR_NOT_SUPPORTED;
            }
            dt_          = a_.src.info_v.datatype;
            dtsz_        = ucc_dt_size(dt_);
            size_t rdtsz = ucc_dt_size(a_.dst.info_v.datatype);
            cnt_.resize(n_);
            dsp_.resize(n_);
            rcnt_.resize(n_);
            rdsp_.resize(n_);
            size_t lmax = 0;
            for (uint32_t r = 0; r < n_; r++) {
                cnt_[r] = coll_count_at(a_, a_.src.info_v.counts, r) *
                          dtsz_;
                dsp_[r] =
                    coll_disp_at(a_, a_.src.info_v.displacements, r) *
                    dtsz_;
                rcnt_[r] = coll_count_at(a_, a_.dst.info_v.counts, r) *
                           rdtsz;
                rdsp_[r] =
                    coll_disp_at(a_, a_.dst.info_v.displacements, r) *
                    rdtsz;
                lmax = cnt_[r] > lmax ? cnt_[r] : lmax;
                lmax = rcnt_[r] > lmax ? rcnt_[r] : lmax;
            }
            sbuf_  = (const uint8_t *)a_.src.info_v.buffer;
            dbuf_  = (uint8_t *)a_.dst.info_v.buffer;
            total_ = lmax; /* provisional; replaced by the global max */
            gran_  = cell_;
            break;
        }
        default:
            return UCC_ERR_NOT_SUPPORTED;
        }
        nfrags_ = (total_ + gran_ - 1) / gran_;
        if (nfrags_ == 0) {
            nfrags_ = 1;
        }
        return UCC_OK;
    }

  public:
    /* zero-copy handle exchange: my src's HIP-IPC handle travels through
     * my scratch in-area (peers read it over the already-mapped IPC
     * scratch), gated by the shm slot steps. One slot use, then the
     * collective itself takes a fresh use. */
    struct ZcBlob {
        uint64_t          magic;
        hipIpcMemHandle_t h;      /* src allocation  */
        uint64_t          base_off;
        uint64_t          raw_ptr;
        hipIpcMemHandle_t hd;     /* dst allocation  */
        uint64_t          d_base_off;
        uint64_t          d_raw_ptr;
        int32_t           pid;
        int32_t           pad;
    };

    ucc_status_t progress() override
    {
        if (phase_ == 20) { /* a2av: publish my local max pair length */
            if (!all_ge(0)) {
                return UCC_INPROGRESS;
            }
            uint64_t mm[2] = {(uint64_t)total_, 0};
            for (uint32_t r = 0; r < n_; r++) {
                mm[1] += cnt_[r]; /* my total send bytes */
            }
            if (hipMemcpy(tt_->area(me_, slot_, 0, 0), mm, sizeof(mm),
                          hipMemcpyHostToDevice) != hipSuccess) {
                return UCC_ERR_NO_RESOURCE;
            }
            publish(1);
            phase_ = 21;
        }
        if (phase_ == 21) { /* a2av: global max + global byte sum */
            if (!all_ge(1)) {
                return UCC_INPROGRESS;
            }
            uint64_t gmax = 0;
            a2av_gsum_    = 0;
            for (uint32_t r = 0; r < n_; r++) {
                uint64_t v[2] = {0, 0};
                if (hipMemcpy(v, tt_->area(r, slot_, 0, 0), sizeof(v),
                              hipMemcpyDeviceToHost) != hipSuccess) {
                    return UCC_ERR_NO_RESOURCE;
                }
                gmax = v[0] > gmax ? v[0] : gmax;
                a2av_gsum_ += v[1];
            }
            total_  = gmax;
            nfrags_ = (total_ + gran_ - 1) / gran_;
            if (nfrags_ == 0) {
                nfrags_ = 1;
            }
            a2av_ready_ = true;
            close_slot();
            begin_use(); /* fresh slot use for the collective itself */
            phase_ = 0;
            /* CE a2av (reference alltoallv_ce.c role): symmetric
             * decision from the GLOBAL byte sum (exchanged with the
             * max), so skewed MoE matrices — whose per-rank totals
             * differ — still get one team-wide verdict. The zc
             * exchange then maps peers' src buffers and their send
             * tables so each rank PULLS its column with SDMA memcpys.
             * SDMA also sidesteps the gated path's worst skew cost:
             * fragment count there scales with the MAX pair length. */
            if (!zc_ready_ && tt_->cfg_.ce_alltoall &&
                Config::instance().get_bool("TL_CDNA4", "ZCOPY", true) &&
                a2av_gsum_ / (n_ ? n_ : 1) >=
                    tt_->cfg_.ce_alltoall_min / 4) {
                zc_    = true;
                phase_ = 10;
            }
        }
        if (phase_ == 10) { /* publish my src handle */
            if (!all_ge(0)) {
                return UCC_INPROGRESS;
            }
            /* what is exported as "my destination": a rank without one
             * (non-root reduce) exports its source again, which takes
             * the same-allocation route below and is never written */
            uint8_t *const xd = dbuf_ ? dbuf_ : (uint8_t *)sbuf_;
            ZcBlob b{};
            b.magic = 0x5a43;
            /* registered-buffer fast path (reference
             * alltoall_onesided.c src_memh/dst_memh role): handles
             * come from the user's ucc_mem_map export instead of a
             * per-post hipIpcGetMemHandle */
            uint64_t moff = 0;
            bool     src_reg =
                (a_.mask & UCC_COLL_ARGS_FIELD_MEM_MAP_SRC_MEMH) &&
                a_.src_memh &&
                ucc_memh_lookup(a_.src_memh, sbuf_, total_, &b.h,
                                &moff);
            if (src_reg) {
                g_memh_uses.fetch_add(1, std::memory_order_relaxed);
                b.base_off = moff;
                b.raw_ptr  = (uint64_t)(uintptr_t)sbuf_;
                b.pid      = (int32_t)getpid();
                uint64_t doff = 0;
                if ((a_.mask &
                     UCC_COLL_ARGS_FIELD_MEM_MAP_DST_MEMH) &&
                    a_.dst_memh &&
                    ucc_memh_lookup(a_.dst_memh, xd, total_, &b.hd,
                                    &doff)) {
                    b.d_base_off = doff;
                    b.d_raw_ptr  = (uint64_t)(uintptr_t)xd;
                    b.pad        = 0;
                } else {
                    /* dst not registered: fall through to the runtime
                     * export for the dst side only */
                    hipDeviceptr_t dbase  = nullptr;
                    size_t         dbsize = 0;
                    if (hipMemGetAddressRange(&dbase, &dbsize,
                                              (hipDeviceptr_t)xd) ==
                            hipSuccess &&
                        hipIpcGetMemHandle(&b.hd, (void *)dbase) ==
                            hipSuccess) {
                        b.d_base_off = (uint64_t)((uintptr_t)xd -
                                                  (uintptr_t)dbase);
                        b.d_raw_ptr  = (uint64_t)(uintptr_t)xd;
                        b.pad        = 0;
                    } else {
                        b.magic = 0;
                        zc_     = false;
                    }
                }
            }
            hipDeviceptr_t base  = nullptr;
            size_t         bsize = 0;
            if (src_reg) {
                /* blob already filled from the registered handles */
            } else if (hipMemGetAddressRange(&base, &bsize,
                                      (hipDeviceptr_t)sbuf_) !=
                    hipSuccess ||
                hipIpcGetMemHandle(&b.h, (void *)base) != hipSuccess) {
                /* MUST stay in the consensus rounds: a unilateral jump
                 * to staging would satisfy peers' all_ge() gates via
                 * close_slot() while they read a stale blob from a
                 * prior use of this rotating slot — silent wrong mode.
                 * Publish a magic=0 blob so the AND-consensus in
                 * phases 11-13 forces every rank to staging. */
                ucc_warn("zero-copy src export failed, using staging");
                zc_ = false;
                b   = ZcBlob{}; /* magic = 0 */
            } else {
                b.base_off =
                    (uint64_t)((uintptr_t)sbuf_ - (uintptr_t)base);
                b.raw_ptr = (uint64_t)(uintptr_t)sbuf_;
                b.pid     = (int32_t)getpid();
                hipDeviceptr_t dbase  = nullptr;
                size_t         dbsize = 0;
                if (ct_ == UCC_COLL_TYPE_ALLTOALLV) {
                    /* CE a2av pulls from peers' src into LOCAL dst:
                     * no dst export needed */
                } else if (hipMemGetAddressRange(&dbase, &dbsize,
                                          (hipDeviceptr_t)xd) ==
                        hipSuccess &&
                    hipIpcGetMemHandle(&b.hd, (void *)dbase) ==
                        hipSuccess) {
                    b.d_base_off =
                        (uint64_t)((uintptr_t)xd - (uintptr_t)dbase);
                    b.d_raw_ptr = (uint64_t)(uintptr_t)xd;
                    b.pad = (dbase == base) ? 1 : 0; /* same alloc */
                } else {
                    b.magic = 0; /* dst export failed: fall back */
                }
            }
            if (hipMemcpy(tt_->area(me_, slot_, 0, 0), &b, sizeof(b),
                          hipMemcpyHostToDevice) != hipSuccess) {
                return UCC_ERR_NO_RESOURCE;
            }
            if (ct_ == UCC_COLL_TYPE_ALLTOALLV) {
                /* publish my send table (byte counts + displs) after
                 * the blob so peers can pull their columns */
                uint64_t tbl[2 * ec_hip::kMaxRanks] = {};
                for (uint32_t r = 0; r < n_; r++) {
                    tbl[r]                      = cnt_[r];
                    tbl[ec_hip::kMaxRanks + r] = dsp_[r];
                }
                if (hipMemcpy(tt_->area(me_, slot_, 0, 0) + 256, tbl,
                              sizeof(tbl),
                              hipMemcpyHostToDevice) != hipSuccess) {
                    return UCC_ERR_NO_RESOURCE;
                }
            }
            publish(1);
            phase_ = 11;
        }
        if (phase_ == 11) { /* open peers' handles */
            if (!all_ge(1)) {
                return UCC_INPROGRESS;
            }
            const bool a2av = ct_ == UCC_COLL_TYPE_ALLTOALLV;
            for (uint32_t r = 0; r < n_ && zc_; r++) {
                if (a2av) { /* read peer r's send table */
                    uint64_t tbl[2 * ec_hip::kMaxRanks];
                    if (hipMemcpy(tbl, tt_->area(r, slot_, 0, 0) + 256,
                                  sizeof(tbl),
                                  hipMemcpyDeviceToHost) != hipSuccess) {
                        zc_ = false;
                        break;
                    }
                    zc_scol_[r] = tbl[me_];
                    zc_sdsp_[r] = tbl[ec_hip::kMaxRanks + me_];
                }
                if (r == me_) {
                    zc_peer_src_[r] = sbuf_;
                    zc_peer_dst_[r] = dbuf_;
                    continue;
                }
                ZcBlob b{};
                if (hipMemcpy(&b, tt_->area(r, slot_, 0, 0), sizeof(b),
                              hipMemcpyDeviceToHost) != hipSuccess ||
                    b.magic != 0x5a43) {
                    ucc_warn("zero-copy import failed, using staging");
                    zc_ = false;
                    break;
                }
                if (b.pid == tt_->team_->ctx->proc.pid) {
                    zc_peer_src_[r] =
                        (const uint8_t *)(uintptr_t)b.raw_ptr;
                    zc_peer_dst_[r] = (uint8_t *)(uintptr_t)b.d_raw_ptr;
                    continue;
                }
                void *m = tt_->ipc_open_cached(
                    b.pid, b.raw_ptr - b.base_off, b.h);
                void *md = nullptr;
                if (!m) {
                    ucc_warn("zero-copy open failed, using staging");
                    zc_ = false;
                    break;
                }
                zc_peer_src_[r] = (const uint8_t *)m + b.base_off;
                if (a2av) {
                    continue; /* pulls land in LOCAL dst */
                }
                md              = tt_->ipc_open_cached(
                    b.pid, b.d_raw_ptr - b.d_base_off, b.hd);
                if (md) {
                    zc_peer_dst_[r] = (uint8_t *)md + b.d_base_off;
                } else if (b.pad == 1) {
                    /* dst lives in the src allocation (e.g. inplace) */
                    zc_peer_dst_[r] =
                        (uint8_t *)m +
                        ((uint64_t)b.d_raw_ptr -
                         ((uint64_t)b.raw_ptr - b.base_off));
                } else {
                    ucc_warn("zero-copy dst open failed, using staging");
                    zc_ = false;
                    break;
                }
            }
            /* direct vector loads/stores need 16B-aligned user
             * buffers on every rank (CE a2av moves bytes with
             * memcpy: exempt) */
            if (zc_ && !a2av) {
                for (uint32_t r = 0; r < n_; r++) {
                    if (((uintptr_t)zc_peer_src_[r] & 15) ||
                        ((uintptr_t)zc_peer_dst_[r] & 15)) {
                        ucc_warn("zero-copy needs 16B-aligned buffers, "
                                 "using staging");
                        zc_ = false;
                        break;
                    }
                }
            }
            publish(2);
            phase_ = 12;
        }
        if (phase_ == 12) { /* blobs consumed -> publish my ok verdict */
            if (!all_ge(2)) {
                return UCC_INPROGRESS;
            }
            /* zero-copy must be ALL-or-nothing: a rank that fell back
             * (export/import/alignment failure) would stage while
             * zero-copy peers read its never-staged areas. Consensus
             * round: everyone posts ok/fail, mode = AND of all. */
            uint64_t ok = zc_ ? 0x5a43u : 0;
            if (hipMemcpy(tt_->area(me_, slot_, 1, 0), &ok, sizeof(ok),
                          hipMemcpyHostToDevice) != hipSuccess) {
                return UCC_ERR_NO_RESOURCE;
            }
            publish(3);
            phase_ = 13;
        }
        if (phase_ == 13) { /* read all verdicts */
            if (!all_ge(3)) {
                return UCC_INPROGRESS;
            }
            for (uint32_t r = 0; r < n_ && zc_; r++) {
                uint64_t ok = 0;
                if (hipMemcpy(&ok, tt_->area(r, slot_, 1, 0), sizeof(ok),
                              hipMemcpyDeviceToHost) != hipSuccess ||
                    ok != 0x5a43u) {
                    zc_ = false;
                }
            }
            if (!zc_) {
                ucc_warn("zero-copy disabled by team consensus, "
                         "using the staged pipeline");
            }
            zc_ready_ = true;
            close_slot();
            begin_use(); /* fresh slot use for the collective itself */
            phase_ = 0;
        }
        if (phase_ == 0) { /* entry: previous use of this slot closed */
            if (!all_ge(0)) {
                return UCC_INPROGRESS;
            }
            done_seq_       = ++tt_->gdone_seq_[slot_];
            ucc_status_t st = enqueue_frags(copy_s(), comp(), false);
            if (st != UCC_OK) {
                return st;
            }
            phase_ = 1;
        }
        /* host-pinned completion flag written by the final kernel once
         * the TEAM's final phase is confirmed (every peer has stopped
         * reading this rank's buffers) — no trailing hipEvent */
        if (*tt_->err_host_ != 0) {
            ucc_error("gated %s timed out waiting for peers",
                      coll_type_name(ct_));
            close_slot();
            return UCC_ERR_TIMED_OUT;
        }
        if (__atomic_load_n(tt_->gdone_host_ + slot_,
                            __ATOMIC_ACQUIRE) < done_seq_) {
            return UCC_INPROGRESS;
        }
        close_slot();
        return UCC_OK;
    }

  private:
    /* SDMA copy-engine alltoall (reference alltoallv_ce.c role): data
     * moves entirely by hipMemcpyAsync pulls over the zero-copy-mapped
     * peer src buffers — the copy engines carry the bytes while the CUs
     * stay free for overlapped compute. Kernels only gate:
     *   [entry signal+reuse waits] -> [all-entered wait] ->
     *   n SDMA pulls on kNumCe streams -> [done signal + team wait]. */
    ucc_status_t enqueue_ce_a2a(hipStream_t comp_s)
    {
        auto *ctx        = (Cdna4TlContext *)tt_->tlc_;
        auto &L          = tt_->gated_launch_;
        const int nblk   = tt_->cfg_.gated_blocks
                               ? tt_->cfg_.gated_blocks
                               : ec_hip::kGatedBlocks;
        const uint64_t B = (uint64_t)nblk;
        const uint32_t p = 0;
        ec_hip::GatedArgs ga{};
        ga.local_flags = tt_->flags_;
        ga.error_word  = tt_->err_host_;
        ga.spin_limit  = tt_->spin_limit();
        ga.nblocks     = nblk;
        ga.pull_wait =
            !Config::instance().get_bool("TL_CDNA4", "PUSH", true);
        ga.rank        = (int)me_;
        ga.nranks      = (int)n_;
        ga.slot        = (int)slot_;
        ga.parity      = (int)p;
        for (uint32_t r = 0; r < n_; r++) {
            ga.peer_flags[r] = tt_->peers_[r].flags;
        }
        ga.len     = 0; /* entry stage is a pure signal */
        ga.n_cells = 0;
        ga.t_sw_reduce  = L[1][slot_][p];
        ga.t_sw_gather  = L[2][slot_][p];
        ga.t_sig_stage  = L[0][slot_][p] + B;
        ga.t_sig_gather = L[2][slot_][p] + B;
        ucc_status_t st = ec_hip::staged_stage(ga, comp_s);
        L[0][slot_][p] += B;
        if (st != UCC_OK) {
            return st;
        }
        /* no peer buffer is written until ITS owner posted (entered) */
        ga.gw_phase      = 0;
        ga.t_gather_wait = L[0][slot_][p];
        st = ec_hip::gated_wait_only(ga, comp_s);
        if (st != UCC_OK) {
            return st;
        }
        HIPCHK(hipEventRecord(ev(8), comp_s));
        bool used[Cdna4TlContext::kNumCe] = {};
        for (uint32_t r = 0; r < n_; r++) {
            /* stagger start peer per rank so SDMA queues don't all hit
             * the same xGMI link first */
            uint32_t rr = (r + me_ + 1) % n_;
            int      si = (int)(r % Cdna4TlContext::kNumCe);
            hipStream_t cs = ctx->ce(si);
            if (!cs) {
                return UCC_ERR_NO_RESOURCE;
            }
            if (!used[si]) {
                HIPCHK(hipStreamWaitEvent(cs, ev(8), 0));
                used[si] = true;
            }
            HIPCHK(hipMemcpyAsync(dbuf_ + (size_t)rr * out_b_,
                                  zc_peer_src_[rr] +
                                      (size_t)me_ * out_b_,
                                  out_b_, hipMemcpyDeviceToDevice, cs));
        }
        for (int si = 0; si < Cdna4TlContext::kNumCe; si++) {
            if (used[si]) {
                HIPCHK(hipEventRecord(ev(9 + si), ctx->ce(si)));
                HIPCHK(hipStreamWaitEvent(comp_s, ev(9 + si), 0));
            }
        }
        /* my pulls done -> publish; complete when every rank's pulls
         * (including reads of MY src) are done */
        ga.t_gather_wait = L[2][slot_][p] + B;
        ga.done_host     = tt_->gdone_host_ + slot_;
        ga.done_seq      = done_seq_;
        st = ec_hip::gated_done(ga, comp_s);
        L[2][slot_][p] += B;
        return st;
    }

    /* CE alltoallv: identical gating to enqueue_ce_a2a; per-peer pull
     * lengths come from the exchanged send tables (len clipped to my
     * recv column, matching the gated a2av semantics). */
    ucc_status_t enqueue_ce_a2av(hipStream_t comp_s)
    {
        auto *ctx        = (Cdna4TlContext *)tt_->tlc_;
        auto &L          = tt_->gated_launch_;
        const int nblk   = tt_->cfg_.gated_blocks
                               ? tt_->cfg_.gated_blocks
                               : ec_hip::kGatedBlocks;
        const uint64_t B = (uint64_t)nblk;
        const uint32_t p = 0;
        ec_hip::GatedArgs ga{};
        ga.local_flags = tt_->flags_;
        ga.error_word  = tt_->err_host_;
        ga.spin_limit  = tt_->spin_limit();
        ga.nblocks     = nblk;
        ga.pull_wait =
            !Config::instance().get_bool("TL_CDNA4", "PUSH", true);
        ga.rank   = (int)me_;
        ga.nranks = (int)n_;
        ga.slot   = (int)slot_;
        ga.parity = (int)p;
        for (uint32_t r = 0; r < n_; r++) {
            ga.peer_flags[r] = tt_->peers_[r].flags;
        }
        ga.len         = 0;
        ga.n_cells     = 0;
        ga.t_sw_reduce  = L[1][slot_][p];
        ga.t_sw_gather  = L[2][slot_][p];
        ga.t_sig_stage  = L[0][slot_][p] + B;
        ga.t_sig_gather = L[2][slot_][p] + B;
        ucc_status_t st = ec_hip::staged_stage(ga, comp_s);
        L[0][slot_][p] += B;
        if (st != UCC_OK) {
            return st;
        }
        ga.gw_phase      = 0;
        ga.t_gather_wait = L[0][slot_][p];
        st = ec_hip::gated_wait_only(ga, comp_s);
        if (st != UCC_OK) {
            return st;
        }
        HIPCHK(hipEventRecord(ev(8), comp_s));
        bool used[Cdna4TlContext::kNumCe] = {};
        for (uint32_t r = 0; r < n_; r++) {
            uint32_t rr  = (r + me_ + 1) % n_;
            uint64_t len = zc_scol_[rr] < rcnt_[rr] ? zc_scol_[rr]
                                                    : rcnt_[rr];
            if (len == 0) {
                continue;
            }
            int         si = (int)(r % Cdna4TlContext::kNumCe);
            hipStream_t cs = ctx->ce(si);
            if (!cs) {
                return UCC_ERR_NO_RESOURCE;
            }
            if (!used[si]) {
                HIPCHK(hipStreamWaitEvent(cs, ev(8), 0));
                used[si] = true;
            }
            HIPCHK(hipMemcpyAsync(dbuf_ + rdsp_[rr],
                                  zc_peer_src_[rr] + zc_sdsp_[rr], len,
                                  hipMemcpyDeviceToDevice, cs));
        }
        for (int si = 0; si < Cdna4TlContext::kNumCe; si++) {
            if (used[si]) {
                HIPCHK(hipEventRecord(ev(9 + si), ctx->ce(si)));
                HIPCHK(hipStreamWaitEvent(comp_s, ev(9 + si), 0));
            }
        }
        ga.t_gather_wait = L[2][slot_][p] + B;
        ga.done_host     = tt_->gdone_host_ + slot_;
        ga.done_seq      = done_seq_;
        st = ec_hip::gated_done(ga, comp_s);
        L[2][slot_][p] += B;
        return st;
    }

    ucc_status_t enqueue_frags(hipStream_t stage_s, hipStream_t comp_s,
                               bool derive)
    {
        if (ct_ == UCC_COLL_TYPE_ALLTOALL && zc_ && zc_ready_ &&
            !derive && tt_->cfg_.ce_alltoall &&
            out_b_ * n_ >= tt_->cfg_.ce_alltoall_min) {
            return enqueue_ce_a2a(comp_s);
        }
        if (ct_ == UCC_COLL_TYPE_ALLTOALLV && zc_ && zc_ready_ &&
            !derive) {
            return enqueue_ce_a2av(comp_s);
        }
        /* bcast / reduce: a triggered post always runs the staged
         * pattern (their zero-copy patterns launch other kernel counts
         * per iteration, the staged one keeps PK_G_AR's pp = 3), so
         * zero-copy state from an earlier host post is ignored and the
         * chunk-sized fragments come back */
        const bool rooted = ct_ == UCC_COLL_TYPE_BCAST ||
                            ct_ == UCC_COLL_TYPE_REDUCE;
        const bool rzc    = rooted && zc_ && zc_ready_ && !derive;
        if (rooted && derive && gran_ != tt_->cfg_.chunk) {
            gran_   = tt_->cfg_.chunk;
            nfrags_ = (total_ + gran_ - 1) / gran_;
            nfrags_ = nfrags_ ? nfrags_ : 1;
        }
        if (zc_ && zc_ready_ && nfrags_ > 1 && !(rooted && derive) &&
            Config::instance().get_bool("TL_CDNA4", "ZC_DEFRAG", true)) {
            /* zero-copy reads/writes USER buffers only — no staging
             * area is touched, so the chunk-size bound (the only reason
             * to fragment) does not apply: one fragment = one
             * stage-signal + reduce + gather per iteration instead of
             * 3 x nfrags launches and their gate waits. Symmetric on
             * every rank (zc is team-consensus). */
            gran_   = total_;
            nfrags_ = 1;
        }
        auto &L          = tt_->gated_launch_;
        /* zero-copy allreduce / reduce_scatter posted from the host:
         * the stage signal, the reduce and the completion wait run as
         * ONE kernel (docs/GATED_PIPELINE.md "Fused zero-copy
         * allreduce"); derive mode keeps the three-kernel pattern its
         * per-block launch arithmetic is built on */
        const bool zc_fused =
            zc_ && zc_ready_ && nfrags_ == 1 && !derive &&
            (ct_ == UCC_COLL_TYPE_ALLREDUCE ||
             ct_ == UCC_COLL_TYPE_REDUCE_SCATTER || rooted) &&
            Config::instance().get_bool("TL_CDNA4", "ZC_FUSED", true);
        /* grid size and cache policy of the data phase: the rule is
         * tl_cdna4::zc_policy (zc_policy.h), measured on the 2-proc rig.
         * 64 blocks by default, 128 from 160 MiB up for a single
         * fragment, and for the one-kernel allreduce of 2 ranks at
         * depth 4 from 128 MiB up 192 blocks and the streamed
         * (non-temporal) data phase (profiles/zc_data_phase.md,
         * profiles/zc_edges_stream.md).
         * Residency: all blocks of a rank spin at entry until every
         * peer's block 0 has run, so the ranks' grids must fit the card
         * together. Every U = 4 instantiation of k_zc_allreduce, plain
         * or streamed, compiles to at least 2 waves/SIMD (VGPRs +
         * AGPRs; `make check-isa`), i.e. 2 blocks of 256 threads per
         * CU, 512 per card, and 192 is below half of that. It does NOT
         * hold at U = 2: the int8/uint8 instantiations there take 256
         * VGPRs plus AGPRs, 1 block per CU, 256 per card, so 3 or 4
         * ranks of 192 blocks on one card could not all be placed.
         * Hence the rule's conditions on n and on the depth the
         * launcher will pick (UCC_EC_REDUCE_DEPTH, like GATED_BLOCKS,
         * has to agree on all ranks: B enters the ledger). The launch
         * ledger accumulates BLOCK counts, so per-collective grids
         * compose on shared (slot,parity) counters; the cache policy
         * does not enter it. */
        const tl_cdna4::ZcColl zct =
            ct_ == UCC_COLL_TYPE_ALLREDUCE        ? tl_cdna4::ZC_COLL_ALLREDUCE
            : ct_ == UCC_COLL_TYPE_REDUCE_SCATTER
                ? tl_cdna4::ZC_COLL_REDUCE_SCATTER
            : ct_ == UCC_COLL_TYPE_REDUCE         ? tl_cdna4::ZC_COLL_REDUCE
            : ct_ == UCC_COLL_TYPE_BCAST          ? tl_cdna4::ZC_COLL_BCAST
                                                  : tl_cdna4::ZC_COLL_OTHER;
        const tl_cdna4::ZcPolicy pol = tl_cdna4::zc_policy(
            zct, zc_fused, (int)n_, ec_hip::zc_depth((int)n_), total_,
            nfrags_ == 1, tt_->cfg_.gated_blocks, tt_->cfg_.zc_stream);
        const int nblk = pol.blocks;
        const uint64_t B = (uint64_t)nblk;
        for (size_t f = 0; f < nfrags_; f++) {
            const uint32_t p   = (uint32_t)(f & 1);
            const size_t   off = f * gran_;
            const size_t   len =
                total_ - off < gran_ ? total_ - off : gran_;
            ec_hip::GatedArgs ga{};
            ga.my_in  = tt_->area(me_, slot_, p, 0);
            ga.my_out = tt_->area(me_, slot_, p, 1);
            for (uint32_t r = 0; r < n_; r++) {
                ga.peer_in[r]    = tt_->area(r, slot_, p, 0);
                ga.peer_out[r]   = tt_->area(r, slot_, p, 1);
                ga.peer_flags[r] = tt_->peers_[r].flags;
            }
            ga.local_flags = tt_->flags_;
            ga.error_word  = tt_->err_host_;
            ga.spin_limit  = tt_->spin_limit();
            ga.nblocks     = nblk;
            ga.pull_wait   = !Config::instance().get_bool(
                "TL_CDNA4", "PUSH", true);
            ga.len         = len;
            ga.rank        = (int)me_;
            ga.nranks      = (int)n_;
            ga.slot        = (int)slot_;
            ga.parity      = (int)p;
            ga.dt          = dt_;
            ga.op          = op_;
            ga.alpha       = alpha_;
            if (derive) {
                const bool is_rs =
                    ct_ == UCC_COLL_TYPE_REDUCE_SCATTER ||
                    ct_ == UCC_COLL_TYPE_REDUCE_SCATTERV;
                const bool ar_pat =
                    ct_ == UCC_COLL_TYPE_ALLREDUCE || rooted;
                ga.derive     = 1;
                ga.pp         = ar_pat ? 3 : 2;
                ga.has_reduce = ar_pat || is_rs;
                ga.has_gather = !is_rs;
            }
            ucc_status_t st = UCC_OK;
            switch (ct_) {
            case UCC_COLL_TYPE_ALLREDUCE: {
                /* stage frag -> reduce my slice -> gather all slices.
                 * zero-copy: stage is a pure signal (len 0) and reduce
                 * reads peers' USER src directly over xGMI */
                ga.src = sbuf_ + off;
                ga.dst = dbuf_ + off;
                size_t per = (len / n_) & ~(size_t)255;
                for (uint32_t r = 0; r < n_; r++) {
                    ga.slice_b[r] = (uint64_t)r * per;
                    ga.slice_e[r] =
                        r == n_ - 1 ? len : (uint64_t)(r + 1) * per;
                }
                ga.sl_b = ga.slice_b[me_];
                ga.sl_e = ga.slice_e[me_];
                if (zc_ && zc_ready_) {
                    /* reduce reads peers' src AND writes every rank's
                     * dst directly; gather becomes a pure wait */
                    ga.len      = 0;
                    ga.zc_write = 1;
                    for (uint32_t r = 0; r < n_; r++) {
                        ga.peer_in[r] = zc_peer_src_[r] + off;
                        ga.peer_out[r] = zc_peer_dst_[r] + off + ga.sl_b;
                    }
                }
                /* zero-copy: stage and gather are pure signal/wait —
                 * a full grid of spinning blocks would only steal CUs
                 * from the reduce; the cumulative-block ledger lets
                 * them launch with ONE block (derive mode keeps the
                 * uniform grid its device-side arithmetic needs). */
                const uint64_t Bs =
                    (!derive && ga.zc_write) ? 1 : B;
                const uint64_t Bg = Bs;
                ga.t_sw_reduce   = L[1][slot_][p];
                ga.t_sw_gather   = L[2][slot_][p];
                ga.t_prev_gather = L[2][slot_][p];
                ga.t_stage       = L[0][slot_][p] + Bs;
                ga.gw_phase      = 1;
                ga.t_gather_wait = L[1][slot_][p] + B;
                ga.t_sig_stage   = L[0][slot_][p] + Bs;
                ga.t_sig_reduce  = L[1][slot_][p] + B;
                ga.t_sig_gather  = L[2][slot_][p] + Bg;
                if (zc_fused) {
                    /* one launch on comp_s: block 0 is the stage
                     * signal, the last-arriving block the completion
                     * wait — same ledger as the three launches */
                    log_path("one-kernel (k_zc_allreduce)", nblk);
                    log_policy(pol.stream);
                    ga.zc_stream = pol.stream ? 1 : 0;
                    ga.done_host = tt_->gdone_host_ + slot_;
                    ga.done_seq  = done_seq_;
                    st = ec_hip::zc_allreduce(ga, comp_s);
                    L[0][slot_][p] += Bs; /* 1 */
                    L[1][slot_][p] += B;
                    L[2][slot_][p] += Bg; /* 1 */
                    break;
                }
                if (ga.zc_write && !derive) {
                    log_path("three-kernel (stage/reduce/gather)", nblk);
                }
                {
                    ec_hip::GatedArgs gs = ga;
                    gs.nblocks           = (int)Bs;
                    st = ec_hip::staged_stage(gs, stage_s);
                }
                if (!derive) { L[0][slot_][p] += Bs; }
                if (st == UCC_OK) {
                    st = ec_hip::staged_reduce(ga, comp_s);
                    if (!derive) { L[1][slot_][p] += B; }
                }
                if (st == UCC_OK) {
                    if (ga.zc_write) {
                        /* dst already written by every rank's reduce:
                         * the gather launch is a pure completion wait */
                        for (uint32_t r = 0; r < n_; r++) {
                            ga.slice_e[r] = ga.slice_b[r];
                        }
                    }
                    ec_hip::GatedArgs gg = ga;
                    gg.nblocks           = (int)Bg;
                    if (!derive && f == nfrags_ - 1) {
                        gg.done_host = tt_->gdone_host_ + slot_;
                        gg.done_seq  = done_seq_;
                    }
                    st = ec_hip::staged_gather(gg, comp_s);
                    if (!derive) { L[2][slot_][p] += Bg; }
                }
                break;
            }
            case UCC_COLL_TYPE_REDUCE:
            case UCC_COLL_TYPE_BCAST: {
                /* Rooted collectives as sub-patterns of the allreduce
                 * (docs/GATED_PIPELINE.md "Rooted collectives"): same
                 * fragments, same slices, and on every rank, whatever
                 * the root, the same launches with the same grids, so
                 * the ledger stays symmetric.
                 *  reduce = allreduce in which only the root gathers;
                 *  bcast  = allreduce with one contributor: rank r takes
                 *           slice r from the root, slices are exchanged. */
                const uint32_t root    = (uint32_t)a_.root;
                const bool     is_root = me_ == root;
                const bool     bc      = ct_ == UCC_COLL_TYPE_BCAST;
                ga.src = sbuf_ + off;
                ga.dst = dbuf_ ? dbuf_ + off : nullptr;
                size_t per = (len / n_) & ~(size_t)255;
                for (uint32_t r = 0; r < n_; r++) {
                    ga.slice_b[r] = (uint64_t)r * per;
                    ga.slice_e[r] =
                        r == n_ - 1 ? len : (uint64_t)(r + 1) * per;
                }
                ga.sl_b = ga.slice_b[me_];
                ga.sl_e = ga.slice_e[me_];
                if (rzc && !bc) {
                    /* zero-copy reduce: the reduce_scatter form. Rank r
                     * reduces slice r of every rank's user src straight
                     * into the ROOT's dst; completion = the team's
                     * reduces are done (root: dst complete; everyone: src
                     * no longer read). In place at the root each slice
                     * is read, then written, by its owner only. */
                    ga.len    = 0;
                    ga.my_out = zc_peer_dst_[root] + off + ga.sl_b;
                    for (uint32_t r = 0; r < n_; r++) {
                        ga.peer_in[r] = zc_peer_src_[r] + off;
                    }
                    ga.t_sw_reduce   = L[1][slot_][p];
                    ga.t_sw_gather   = L[2][slot_][p];
                    ga.t_prev_gather = 0;
                    ga.t_stage       = L[0][slot_][p] + 1;
                    ga.t_sig_stage   = L[0][slot_][p] + 1;
                    ga.t_sig_reduce  = L[1][slot_][p] + B;
                    if (zc_fused) {
                        log_path("one-kernel (k_zc_allreduce into the "
                                 "root's dst)", nblk);
                        log_policy(pol.stream);
                        ga.zc_stream     = pol.stream ? 1 : 0;
                        ga.t_gather_wait = L[1][slot_][p] + B;
                        ga.done_host     = tt_->gdone_host_ + slot_;
                        ga.done_seq      = done_seq_;
                        st = ec_hip::zc_allreduce(ga, comp_s);
                        L[0][slot_][p] += 1;
                        L[1][slot_][p] += B;
                        break;
                    }
                    log_path("three-kernel (stage/reduce/wait into the "
                             "root's dst)", nblk);
                    {
                        ec_hip::GatedArgs gs = ga;
                        gs.nblocks           = 1;
                        st = ec_hip::staged_stage(gs, stage_s);
                    }
                    L[0][slot_][p] += 1;
                    if (st == UCC_OK) {
                        st = ec_hip::staged_reduce(ga, comp_s);
                        L[1][slot_][p] += B;
                    }
                    if (st == UCC_OK && f == nfrags_ - 1) {
                        ec_hip::GatedArgs gw = ga;
                        gw.gw_phase          = 1;
                        gw.t_gather_wait     = L[1][slot_][p];
                        gw.done_host         = tt_->gdone_host_ + slot_;
                        gw.done_seq          = done_seq_;
                        st = ec_hip::gated_wait_only(gw, comp_s);
                    }
                    break;
                }
                if (rzc) {
                    /* zero-copy bcast, push: rank r reads slice r of the
                     * root's user buffer and writes it into every
                     * non-root rank's buffer at the same offset (the
                     * root's own entry stays null: skipped) */
                    ga.len        = 0;
                    ga.zc_write   = 1;
                    ga.peer_in[0] = zc_peer_src_[root] + off;
                    for (uint32_t r = 0; r < n_; r++) {
                        ga.peer_out[r] =
                            r == root ? nullptr
                                      : (const void *)(zc_peer_dst_[r] +
                                                       off + ga.sl_b);
                    }
                }
                /* allreduce targets and increments: full grids when
                 * staged (and always in derive mode), one block for the
                 * pure signal / pure wait of the zero-copy form */
                const uint64_t Bs = rzc ? 1 : B;
                const uint64_t Bg = Bs;
                ga.t_sw_reduce   = L[1][slot_][p];
                ga.t_sw_gather   = L[2][slot_][p];
                ga.t_prev_gather = L[2][slot_][p];
                ga.t_stage       = L[0][slot_][p] + Bs;
                ga.gw_phase      = 1;
                ga.t_gather_wait = L[1][slot_][p] + B;
                ga.t_sig_stage   = L[0][slot_][p] + Bs;
                ga.t_sig_reduce  = L[1][slot_][p] + B;
                ga.t_sig_gather  = L[2][slot_][p] + Bg;
                if (rzc && zc_fused) {
                    log_path("one-kernel (k_zc_bcast)", nblk);
                    ga.done_host = tt_->gdone_host_ + slot_;
                    ga.done_seq  = done_seq_;
                    st = ec_hip::zc_bcast(ga, comp_s);
                    L[0][slot_][p] += 1;
                    L[1][slot_][p] += B;
                    L[2][slot_][p] += 1;
                    break;
                }
                if (rzc) {
                    log_path("three-kernel (stage/bscatter/wait)", nblk);
                }
                {
                    /* staged: every rank of a reduce stages its fragment,
                     * of a bcast the root alone (the others only signal) */
                    ec_hip::GatedArgs gs = ga;
                    gs.nblocks           = (int)Bs;
                    if (!rzc && bc && !is_root) {
                        gs.len = 0;
                    }
                    st = ec_hip::staged_stage(gs, stage_s);
                }
                if (!derive) { L[0][slot_][p] += Bs; }
                if (st == UCC_OK) {
                    if (bc) {
                        ec_hip::GatedArgs gb = ga;
                        if (!rzc) {
                            /* my slice of the ROOT's in-area -> my out */
                            gb.peer_in[0] = tt_->area(root, slot_, p, 0);
                        }
                        st = ec_hip::staged_bscatter(gb, comp_s);
                    } else {
                        st = ec_hip::staged_reduce(ga, comp_s);
                    }
                    if (!derive) { L[1][slot_][p] += B; }
                }
                if (st == UCC_OK) {
                    /* who gathers: of a reduce the root, of a bcast
                     * everyone else; all other launches (and all of the
                     * zero-copy form) are wait + signal only */
                    ec_hip::GatedArgs gg = ga;
                    gg.nblocks           = (int)Bg;
                    if (rzc || (bc ? is_root : !is_root)) {
                        for (uint32_t r = 0; r < n_; r++) {
                            gg.slice_e[r] = gg.slice_b[r];
                        }
                    }
                    if (!derive && f == nfrags_ - 1) {
                        gg.done_host = tt_->gdone_host_ + slot_;
                        gg.done_seq  = done_seq_;
                    }
                    st = ec_hip::staged_gather(gg, comp_s);
                    if (!derive) { L[2][slot_][p] += Bg; }
                }
                break;
            }
            case UCC_COLL_TYPE_REDUCE_SCATTERV:
            case UCC_COLL_TYPE_REDUCE_SCATTER: {
                /* stage frag of the whole source; reduce ONLY the
                 * intersection with my output slice, directly into my
                 * user dst (no gather phase) */
                ga.src = sbuf_ + off;
                size_t s0, s1;
                if (ct_ == UCC_COLL_TYPE_REDUCE_SCATTERV) {
                    s0 = dsp_[me_];
                    s1 = s0 + cnt_[me_];
                } else {
                    s0 = (size_t)me_ * out_b_;
                    s1 = s0 + out_b_;
                }
                size_t b = s0 > off ? s0 : off;
                size_t e = s1 < off + len ? s1 : off + len;
                ga.sl_b   = b > e ? 0 : b - off;
                ga.sl_e   = b > e ? 0 : e - off;
                ga.my_out = dbuf_ + (b >= s0 && b <= s1 ? b - s0 : 0);
                if (zc_ && zc_ready_) {
                    /* reduce reads peers' user src directly */
                    ga.len = 0;
                    for (uint32_t r = 0; r < n_; r++) {
                        ga.peer_in[r] = zc_peer_src_[r] + off;
                    }
                }
                const uint64_t Bs =
                    (!derive && zc_ && zc_ready_) ? 1 : B;
                ga.t_sw_reduce   = L[1][slot_][p];
                ga.t_sw_gather   = L[2][slot_][p];
                ga.t_prev_gather = 0;
                ga.t_stage       = L[0][slot_][p] + Bs;
                ga.t_sig_stage   = L[0][slot_][p] + Bs;
                ga.t_sig_reduce  = L[1][slot_][p] + B;
                if (zc_fused) {
                    /* same kernel, zc_write = 0: my slice into my dst
                     * only, team-reduces-done wait, no phase 2 */
                    log_path("one-kernel (k_zc_allreduce)", nblk);
                    log_policy(pol.stream);
                    ga.zc_stream     = pol.stream ? 1 : 0;
                    ga.t_gather_wait = L[1][slot_][p] + B;
                    ga.done_host     = tt_->gdone_host_ + slot_;
                    ga.done_seq      = done_seq_;
                    st = ec_hip::zc_allreduce(ga, comp_s);
                    L[0][slot_][p] += Bs; /* 1 */
                    L[1][slot_][p] += B;
                    break;
                }
                if (zc_ && zc_ready_ && !derive) {
                    log_path("three-kernel (stage/reduce/wait)", nblk);
                }
                {
                    ec_hip::GatedArgs gs = ga;
                    gs.nblocks           = (int)Bs;
                    st = ec_hip::staged_stage(gs, stage_s);
                }
                if (!derive) { L[0][slot_][p] += Bs; }
                if (st == UCC_OK) {
                    st = ec_hip::staged_reduce(ga, comp_s);
                    if (!derive) { L[1][slot_][p] += B; }
                }
                if (st == UCC_OK && !derive && f == nfrags_ - 1) {
                    /* completion = the TEAM's reduces done: a peer's
                     * zero-copy reduce may still be reading MY src
                     * when my own reduce retires */
                    ec_hip::GatedArgs gw = ga;
                    gw.gw_phase          = 1;
                    gw.t_gather_wait     = L[1][slot_][p];
                    gw.done_host         = tt_->gdone_host_ + slot_;
                    gw.done_seq          = done_seq_;
                    st = ec_hip::gated_wait_only(gw, comp_s);
                }
                break;
            }
            case UCC_COLL_TYPE_ALLGATHERV:
            case UCC_COLL_TYPE_ALLGATHER: {
                /* stage my block frag; gather reads peers' STAGED data
                 * (in areas) into dst block positions. v: per-rank
                 * lengths clipped to each block's count */
                size_t mylen =
                    off >= cnt_[me_] ? 0
                    : cnt_[me_] - off < gran_ ? cnt_[me_] - off
                                              : gran_;
                ga.src = sbuf_ + off;
                ga.len = mylen;
                ga.dst = dbuf_;
                const bool agzc = zc_ && zc_ready_;
                if (agzc) {
                    ga.len = 0; /* stage = pure signal */
                    log_path("gather from the peers' user src", (int)B);
                }
                for (uint32_t r = 0; r < n_; r++) {
                    ga.peer_out[r] =
                        agzc ? (const void *)(zc_peer_src_[r] + off)
                             : (const void *)tt_->area(r, slot_, p, 0);
                    size_t l = off >= cnt_[r] ? 0
                               : cnt_[r] - off < gran_ ? cnt_[r] - off
                                                       : gran_;
                    ga.slice_b[r] = dsp_[r] + off;
                    ga.slice_e[r] = ga.slice_b[r] + l;
                }
                const uint64_t Bs =
                    (!derive && agzc) ? 1 : B;
                ga.t_sw_reduce   = L[1][slot_][p];
                ga.t_sw_gather   = L[2][slot_][p];
                ga.gw_phase      = 0;
                ga.t_gather_wait = L[0][slot_][p] + Bs;
                ga.t_sig_stage   = L[0][slot_][p] + Bs;
                ga.t_sig_gather  = L[2][slot_][p] + B;
                {
                    ec_hip::GatedArgs gs = ga;
                    gs.nblocks           = (int)Bs;
                    st = ec_hip::staged_stage(gs, stage_s);
                }
                if (!derive) { L[0][slot_][p] += Bs; }
                if (st == UCC_OK) {
                    st = ec_hip::staged_gather(ga, comp_s);
                    if (!derive) { L[2][slot_][p] += B; }
                }
                if (st == UCC_OK && !derive && f == nfrags_ - 1) {
                    ec_hip::GatedArgs gw = ga;
                    gw.gw_phase          = 2;
                    gw.t_gather_wait     = L[2][slot_][p];
                    gw.done_host         = tt_->gdone_host_ + slot_;
                    gw.done_seq          = done_seq_;
                    st = ec_hip::gated_wait_only(gw, comp_s);
                }
                break;
            }
            case UCC_COLL_TYPE_ALLTOALLV: {
                /* per-dest cells with per-pair lengths: send cells clip
                 * to my send row, gather slices clip to my recv column.
                 * Fragment count is the exchanged GLOBAL max, so every
                 * rank launches identically (ledger stays in sync). */
                ga.src     = sbuf_;
                ga.dst     = dbuf_;
                ga.n_cells = (int)n_;
                for (uint32_t r = 0; r < n_; r++) {
                    size_t sl = off >= cnt_[r] ? 0
                                : cnt_[r] - off < gran_ ? cnt_[r] - off
                                                        : gran_;
                    size_t rl = off >= rcnt_[r] ? 0
                                : rcnt_[r] - off < gran_
                                    ? rcnt_[r] - off
                                    : gran_;
                    ga.c_src_off[r] = dsp_[r] + off;
                    ga.c_dst_off[r] = (uint64_t)r * cell_;
                    ga.c_len[r]     = sl;
                    ga.peer_out[r] =
                        (const void *)(tt_->area(r, slot_, p, 0) +
                                       me_ * cell_);
                    ga.slice_b[r] = rdsp_[r] + off;
                    ga.slice_e[r] = ga.slice_b[r] + rl;
                }
                ga.t_sw_reduce   = L[1][slot_][p];
                ga.t_sw_gather   = L[2][slot_][p];
                ga.gw_phase      = 0;
                ga.t_gather_wait = L[0][slot_][p] + B;
                ga.t_sig_stage   = L[0][slot_][p] + B;
                ga.t_sig_gather  = L[2][slot_][p] + B;
                st = ec_hip::staged_stage(ga, stage_s);
                if (!derive) { L[0][slot_][p] += B; }
                if (st == UCC_OK) {
                    st = ec_hip::staged_gather(ga, comp_s);
                    if (!derive) { L[2][slot_][p] += B; }
                }
                if (st == UCC_OK && !derive && f == nfrags_ - 1) {
                    ec_hip::GatedArgs gw = ga;
                    gw.gw_phase          = 2;
                    gw.t_gather_wait     = L[2][slot_][p];
                    gw.done_host         = tt_->gdone_host_ + slot_;
                    gw.done_seq          = done_seq_;
                    st = ec_hip::gated_wait_only(gw, comp_s);
                }
                break;
            }
            case UCC_COLL_TYPE_ALLTOALL: {
                /* stage per-dest cells; gather my cell from each peer.
                 * zero-copy: gather reads peers' USER src at my block's
                 * offset directly; stage = pure signal */
                ga.src     = sbuf_;
                ga.dst     = dbuf_;
                const bool a2zc = zc_ && zc_ready_;
                ga.n_cells = a2zc ? 0 : (int)n_;
                if (a2zc) {
                    ga.len = 0; /* stage = pure signal */
                    log_path("gather from the peers' user src", (int)B);
                }
                for (uint32_t r = 0; r < n_; r++) {
                    ga.c_src_off[r] = (uint64_t)r * out_b_ + off;
                    ga.c_dst_off[r] = (uint64_t)r * cell_;
                    ga.c_len[r]     = a2zc ? 0 : len;
                    ga.peer_out[r] =
                        a2zc ? (const void *)(zc_peer_src_[r] +
                                              me_ * out_b_ + off)
                             : (const void *)(tt_->area(r, slot_, p, 0) +
                                              me_ * cell_);
                    ga.slice_b[r] = (uint64_t)r * out_b_ + off;
                    ga.slice_e[r] = ga.slice_b[r] + len;
                }
                const uint64_t Bs =
                    (!derive && a2zc) ? 1 : B;
                ga.t_sw_reduce   = L[1][slot_][p];
                ga.t_sw_gather   = L[2][slot_][p];
                ga.gw_phase      = 0;
                ga.t_gather_wait = L[0][slot_][p] + Bs;
                ga.t_sig_stage   = L[0][slot_][p] + Bs;
                ga.t_sig_gather  = L[2][slot_][p] + B;
                {
                    ec_hip::GatedArgs gs = ga;
                    gs.nblocks           = (int)Bs;
                    st = ec_hip::staged_stage(gs, stage_s);
                }
                if (!derive) { L[0][slot_][p] += Bs; }
                if (st == UCC_OK) {
                    st = ec_hip::staged_gather(ga, comp_s);
                    if (!derive) { L[2][slot_][p] += B; }
                }
                if (st == UCC_OK && !derive && f == nfrags_ - 1) {
                    ec_hip::GatedArgs gw = ga;
                    gw.gw_phase          = 2;
                    gw.t_gather_wait     = L[2][slot_][p];
                    gw.done_host         = tt_->gdone_host_ + slot_;
                    gw.done_seq          = done_seq_;
                    st = ec_hip::gated_wait_only(gw, comp_s);
                }
                break;
            }
            default:
                return UCC_ERR_NOT_SUPPORTED;
            }
            if (st != UCC_OK) {
                return st;
            }
        }
        return UCC_OK;
    }

    ucc_coll_type_t    ct_    = UCC_COLL_TYPE_ALLREDUCE;
    ucc_datatype_t     dt_    = UCC_DT_FLOAT32;
    ucc_reduction_op_t op_    = UCC_OP_SUM;
    double             alpha_ = 1.0;
    size_t             dtsz_ = 4, total_ = 0, nfrags_ = 0;
    size_t             gran_ = 0, cell_ = 0, out_b_ = 0;
    const uint8_t     *sbuf_ = nullptr;
    uint8_t           *dbuf_ = nullptr;
    std::vector<size_t> cnt_, dsp_;   /* send row bytes (ag/rs/a2av)  */
    std::vector<size_t> rcnt_, rdsp_; /* recv column bytes (a2av)     */
    bool                a2av_ready_ = false; /* global max exchanged  */
    uint64_t            a2av_gsum_  = 0;     /* global send-byte sum  */
    uint64_t            done_seq_   = 0;     /* host completion seq   */
    bool                path_logged_ = false;

    /* one debug line per task naming the zero-copy launch pattern */
    void log_path(const char *path, int nblk)
    {
        if (!path_logged_) {
            path_logged_ = true;
            ucc_debug("cdna4 gated %s: zero-copy %s path, %d blocks, "
                      "%zu bytes", coll_type_name(ct_), path, nblk,
                      (size_t)total_);
        }
    }
    /* and one naming the cache policy of k_zc_allreduce's data phase:
     * what zc_policy returned, and whether the knob had asked for more */
    void log_policy(bool stream)
    {
        if (!policy_logged_) {
            policy_logged_ = true;
            const bool want = tt_->cfg_.zc_stream == tl_cdna4::ZC_STREAM_ON;
            ucc_debug("cdna4 gated %s: zc data phase: %s",
                      coll_type_name(ct_),
                      stream ? "streaming"
                      : want ? "plain (no streamed instantiation)"
                             : "plain");
        }
    }
    bool               policy_logged_ = false;
    int                pslot_ = -1;
    /* zero-copy persistent allreduce: peers' USER src buffers mapped
     * via HIP-IPC (handles exchanged through the scratch channel at
     * first post) — the reduce phase reads them directly, the stage
     * kernel degenerates to a pure signal (no staging copy). */
    bool               zc_ = false, zc_ready_ = false;
    const uint8_t     *zc_peer_src_[ec_hip::kMaxRanks] = {};
    uint8_t           *zc_peer_dst_[ec_hip::kMaxRanks] = {};
    /* CE a2av: peer r's send-to-me byte count / displacement */
    uint64_t           zc_scol_[ec_hip::kMaxRanks] = {};
    uint64_t           zc_sdsp_[ec_hip::kMaxRanks] = {};

  public:
    ~GatedCollTask() override
    {
        if (pslot_ >= 0) {
            tt_->free_pslot(pslot_);
        }
        /* zero-copy imports stay in the team cache (ipc_open_cached) */
    }
};

/* Host-gated multi-ring reduce_scatter / allgather / allreduce: the
 * link-partitioned alternative to the direct (staged_linear,
 * gated_pipeline) algorithms, opt-in through UCC_TL_CDNA4_RING. The
 * schedule is ring_plan.h; this task resolves its offsets to pointers and
 * drives it the way StagedTask drives its phases: one ec_hip::ring_step
 * launch per step on comp(), each gated ON THE HOST on the shm step
 * counters of the ring neighbours, hand-offs at kernel boundaries only. The
 * kernel never waits, so the in-process jig runs it at any rank count and a
 * dead peer ends as a request timeout.
 *
 * The outbox of parity p is area(me, slot, p, 0); the travelling partial
 * stays in accumulator type (f32 for the 8/16-bit floats), which is why
 * the fragment width is chunk / sizeof(acc). Launch g publishes g + 1 once
 * its event has completed. Launch 0 waits for ALL ranks to have closed the
 * slot's previous use, like every staged task: that use may have been a
 * direct algorithm, whose readers are not only the ring neighbours. */
class RingTask final : public Cdna4Task {
  public:
    using Cdna4Task::Cdna4Task;

    /* what of `a` the plan needs; false: not a ring collective */
    struct Shape {
        RingColl       coll;
        bool           inplace;
        ucc_datatype_t dt;
        uint64_t       count; /* per rank (rs, ag) or whole vector (ar) */
        size_t         dtsz, accsz;
        const uint8_t *sbuf;
        uint8_t       *dbuf;
    };
    static bool shape_of(const ucc_coll_args_t &a, uint32_t me, uint32_t n,
                         Shape *s)
    {
        s->inplace = a.flags & UCC_COLL_ARGS_FLAG_IN_PLACE;
        s->dt      = a.dst.info.datatype;
        if (!ucc_dt_is_predefined(s->dt)) {
            return false;
        }
        s->dtsz = ucc_dt_size(s->dt);
        uint8_t       *dst = (uint8_t *)a.dst.info.buffer;
        const uint8_t *src = (const uint8_t *)a.src.info.buffer;
        switch (a.coll_type) {
        case UCC_COLL_TYPE_ALLREDUCE:
            s->coll  = RING_ALLREDUCE;
            s->count = a.dst.info.count;
            s->dbuf  = dst;
            s->sbuf  = s->inplace ? dst : src;
            break;
        case UCC_COLL_TYPE_REDUCE_SCATTER:
            s->coll = RING_REDUCE_SCATTER;
            if (s->inplace) {
                s->count = a.dst.info.count / n;
                s->sbuf  = dst;
                s->dbuf  = dst + (size_t)me * s->count * s->dtsz;
            } else {
                s->count = a.dst.info.count;
                s->sbuf  = src;
                s->dbuf  = dst;
            }
            break;
        case UCC_COLL_TYPE_ALLGATHER:
            /* pure data movement: planned and copied as bytes */
            s->coll  = RING_ALLGATHER;
            s->count = a.dst.info.count * s->dtsz / n;
            s->dt    = UCC_DT_UINT8;
            s->dtsz  = 1;
            s->dbuf  = dst;
            s->sbuf  = s->inplace ? dst + (size_t)me * s->count : src;
            break;
        default: return false;
        }
        if (s->coll != RING_ALLGATHER) {
            /* complex SUM / AVG: float on 2x the elements */
            const bool c32 = s->dt == UCC_DT_FLOAT32_COMPLEX;
            const bool c64 = s->dt == UCC_DT_FLOAT64_COMPLEX;
            if ((c32 || c64) &&
                (a.op == UCC_OP_SUM || a.op == UCC_OP_AVG)) {
                s->dt = c32 ? UCC_DT_FLOAT32 : UCC_DT_FLOAT64;
                s->count *= 2;
                s->dtsz /= 2;
            }
        }
        const bool narrow =
            s->dt == UCC_DT_BFLOAT16 || s->dt == UCC_DT_FLOAT16 ||
            s->dt == UCC_DT_FLOAT8_E4M3 || s->dt == UCC_DT_FLOAT8_E5M2;
        s->accsz = narrow ? sizeof(float) : s->dtsz;
        return true;
    }

    /* init-time check: everything post() relies on, so that a refusal
     * happens before the request takes a place in the post order */
    static bool supported(const ucc_coll_args_t &a, Cdna4TlTeam *tt)
    {
        Shape    s;
        RingPlan p;
        const uint32_t n = tt->team_->size;
        if (!shape_of(a, tt->team_->rank, n, &s)) {
            return false;
        }
        if (s.coll != RING_ALLGATHER && !ec_hip::op_supported(s.dt, a.op)) {
            return false;
        }
        return ring_plan_init(&p, (int)n, (int)tt->team_->rank,
                              tt->cfg_.ring_nrings, s.coll, s.inplace,
                              s.count, s.dtsz, s.accsz, tt->cfg_.chunk) &&
               ring_plan_launches(p) + 1 < kCap;
    }

    ucc_status_t post() override
    {
        begin_use();
        if (!shape_of(a_, me_, n_, &s_) ||
            !ring_plan_init(&plan_, (int)n_, (int)me_, tt_->cfg_.ring_nrings,
                            s_.coll, s_.inplace, s_.count, s_.dtsz, s_.accsz,
                            tt_->cfg_.chunk)) {
            return UCC_ERR_NOT_SUPPORTED; /* supported() said otherwise */
        }
        op_    = a_.op;
        alpha_ = 1.0;
        if (op_ == UCC_OP_AVG) {
            op_    = (ucc_reduction_op_t)12; /* SUM + alpha */
            alpha_ = 1.0 / (double)n_;
        }
        n_nb_     = ring_plan_neighbours(plan_, nb_);
        total_    = ring_plan_launches(plan_);
        g_        = 0;
        launched_ = false;
        status    = UCC_INPROGRESS;
        return progress();
    }

    ucc_status_t progress() override
    {
        while (g_ < total_) {
            if (!launched_) {
                if (!gate()) {
                    return UCC_INPROGRESS;
                }
                ucc_status_t st = launch();
                if (st != UCC_OK) {
                    close_slot();
                    return st;
                }
                HIPWARN(hipEventRecord(ev(0), comp()));
                launched_ = true;
            }
            hipError_t e = hipEventQuery(ev(0));
            if (e == hipErrorNotReady) {
                return UCC_INPROGRESS;
            }
            if (e != hipSuccess) {
                close_slot();
                return UCC_ERR_NO_RESOURCE;
            }
            launched_ = false;
            g_++;
            publish(g_);
        }
        close_slot();
        return UCC_OK;
    }

  private:
    bool gate()
    {
        if (g_ == 0) {
            return all_ge(0);
        }
        for (int i = 0; i < n_nb_; i++) {
            if (tt_->seg_.step(slot_, (uint32_t)nb_[i])
                    ->load(std::memory_order_acquire) < base_ + g_) {
                return false;
            }
        }
        return true;
    }

    ucc_status_t launch()
    {
        RingLaunch l;
        ring_plan_launch(plan_, g_ / (uint64_t)plan_.L,
                         (int)(g_ % (uint64_t)plan_.L), &l);
        const size_t in_sz  = l.in_acc ? s_.accsz : s_.dtsz;
        const size_t out_sz = l.out_acc ? s_.accsz : s_.dtsz;
        ec_hip::RingStepArgs ra{};
        ra.n_rings = l.npieces;
        ra.dt      = s_.dt;
        ra.op      = op_;
        ra.alpha   = l.final_rs ? alpha_ : 1.0;
        ra.in_acc  = l.in_acc;
        ra.out_acc = l.out_acc;
        ra.nblocks = 0;
        uint8_t *outbox = tt_->area(me_, slot_, (uint32_t)l.out_parity, 0);
        for (int k = 0; k < l.npieces; k++) {
            const RingPieceDesc &d  = l.p[k];
            ec_hip::RingPiece   &pc = ra.piece[k];
            pc.count                = d.count;
            if (d.count == 0) {
                continue;
            }
            if (l.in_from_src) {
                pc.in = s_.sbuf + d.src_off * s_.dtsz;
            } else if (l.use_in) {
                pc.in = tt_->area((uint32_t)d.left, slot_,
                                  (uint32_t)l.in_parity, 0) +
                        d.box_off * in_sz;
            }
            if (l.use_local) {
                pc.local = s_.sbuf + d.src_off * s_.dtsz;
            }
            if (l.use_out) {
                pc.out = outbox + d.box_off * out_sz;
            }
            if (l.use_dst) {
                pc.dst = s_.dbuf + d.dst_off * s_.dtsz;
            }
        }
        return ec_hip::ring_step(ra, comp());
    }

    Shape              s_{};
    RingPlan           plan_;
    ucc_reduction_op_t op_    = UCC_OP_SUM;
    double             alpha_ = 1.0;
    int                nb_[2 * kRingMaxRings] = {};
    int                n_nb_     = 0;
    uint64_t           total_    = 0, g_ = 0;
    bool               launched_ = false;
};

/* Device active-set bcast: a transfer of one device buffer from `root` to
 * the other members of the strided rank subset {start, stride, size}. A
 * 2-member set with the sender as root is a send/recv (reference: tl/ucp
 * active-set bcast, the p2p that pipeline stages ride on).
 *
 * Non-members post nothing, so this task takes no part in the team-wide
 * post order: no begin_use(), no seq_, no rotating or persistent slot, no
 * gated_launch_. Its control channel is the per-pair mailbox
 * (p2p_mbox.h): the root publishes one descriptor (length, tag, IPC handle
 * of the source) per other member and launches nothing; each member waits
 * ON THE HOST for its descriptor, then pulls the bytes with one
 * k_p2p_pull launch, polls the host-pinned completion word and acks. The
 * kernel never waits, so several ranks of one process on one hardware
 * queue are safe and a dead peer cannot hang the device.
 *
 * Ordering: on one ordered pair transfers match in post order
 * (non-overtaking); different pairs are independent. Tags are verified,
 * not searched for. Host-post semantics: the source must be complete when
 * the root posts. */
class ActiveSetBcastTask final : public Cdna4Task {
  public:
    using Cdna4Task::Cdna4Task;

    ucc_status_t post() override
    {
        me_    = tt_->team_->rank;
        n_     = tt_->team_->size;
        bytes_ = a_.src.info.count * ucc_dt_size(a_.src.info.datatype);
        root_  = (uint32_t)a_.root;
        /* member list: tl/tcp's arithmetic */
        bool me_in = false, root_in = false;
        std::vector<uint32_t> set;
        for (int64_t i = 0; i < (int64_t)a_.active_set.size; i++) {
            uint32_t r = (uint32_t)(((a_.active_set.start +
                                      i * a_.active_set.stride) %
                                         (int64_t)n_ +
                                     (int64_t)n_) %
                                    (int64_t)n_);
            me_in |= r == me_;
            root_in |= r == root_;
            bool dup = false;
            for (uint32_t s : set) {
                dup |= s == r;
            }
            if (!dup) {
                set.push_back(r);
            }
        }
        if (!me_in || !root_in || a_.root >= n_) {
            return UCC_ERR_INVALID_PARAM; /* caller or root not in the set */
        }
        std::lock_guard<std::mutex> g(tt_->p2p_mu_);
        dsts_.clear();
        if (me_ == root_) {
            for (uint32_t r : set) {
                if (r != me_) {
                    dsts_.push_back(Dst{r, ++tt_->p2p_send_seq_[r], false,
                                        false});
                }
            }
            if (!exported_) {
                export_src();
            }
        } else {
            seq_ = ++tt_->p2p_recv_seq_[root_];
        }
        phase_  = 0;
        result_ = UCC_OK;
        status  = UCC_INPROGRESS;
        return step();
    }

    ucc_status_t progress() override
    {
        std::lock_guard<std::mutex> g(tt_->p2p_mu_);
        return step();
    }

  private:
    struct Dst {
        uint32_t rank;
        uint64_t seq;
        bool     published, acked;
    };

    /* root: IPC handle of the source allocation, once per request. Only
     * needed when a member lives in another process. A failure travels in
     * the descriptor so that the member fails too instead of waiting. */
    void export_src()
    {
        exported_ = true;
        tmpl_     = P2pDesc{};
        tmpl_.len     = bytes_;
        tmpl_.raw_ptr = (uint64_t)(uintptr_t)a_.src.info.buffer;
        tmpl_.pid     = (int32_t)getpid();
        tmpl_.has_tag = (a_.mask & UCC_COLL_ARGS_FIELD_TAG) ? 1 : 0;
        tmpl_.tag     = tmpl_.has_tag ? a_.tag : 0;
        bool remote = false;
        for (auto &d : dsts_) {
            remote |= tt_->team_->procs[d.rank].pid != tmpl_.pid;
        }
        if (!remote || bytes_ == 0) {
            return;
        }
        uint64_t moff = 0;
        if ((a_.mask & UCC_COLL_ARGS_FIELD_MEM_MAP_SRC_MEMH) &&
            a_.src_memh &&
            ucc_memh_lookup(a_.src_memh, a_.src.info.buffer, bytes_,
                            tmpl_.handle, &moff)) {
            g_memh_uses.fetch_add(1, std::memory_order_relaxed);
            tmpl_.base_off   = moff;
            tmpl_.has_handle = 1;
            return;
        }
        hipDeviceptr_t    base  = nullptr;
        size_t            bsize = 0;
        hipIpcMemHandle_t h;
        static_assert(sizeof(h) == sizeof(tmpl_.handle), "IPC handle size");
        if (hipMemGetAddressRange(&base, &bsize,
                                  (hipDeviceptr_t)a_.src.info.buffer) !=
                hipSuccess ||
            hipIpcGetMemHandle(&h, (void *)base) != hipSuccess) {
            (void)hipGetLastError();
            ucc_error("active-set bcast: cannot export source %p for IPC",
                      a_.src.info.buffer);
            tmpl_.status = (int32_t)UCC_ERR_NO_RESOURCE;
            return;
        }
        memcpy(tmpl_.handle, &h, sizeof(h));
        tmpl_.base_off =
            (uint64_t)((uintptr_t)a_.src.info.buffer - (uintptr_t)base);
        tmpl_.has_handle = 1;
    }

    ucc_status_t step() { return me_ == root_ ? step_root() : step_member(); }

    /* root: publish in channel order (ring full: retry from progress),
     * then collect the acks; first error status wins */
    ucc_status_t step_root()
    {
        P2pMbox &mb   = tt_->mbox_;
        bool     done = true;
        for (auto &d : dsts_) {
            if (!d.published) {
                /* the ack status slot of seq - D is rewritten once seq is
                 * acked: post only after its owner has read it */
                if (!mb.can_post(me_, d.rank, d.seq) ||
                    d.seq - tt_->p2p_send_read_[d.rank] > mb.depth()) {
                    done = false;
                    continue;
                }
                P2pDesc desc = tmpl_;
                desc.seq     = d.seq;
                mb.post(me_, d.rank, desc);
                d.published = true;
            }
            if (!d.acked) {
                int32_t st = 0;
                if (tt_->p2p_send_read_[d.rank] + 1 != d.seq ||
                    !mb.ack_of(me_, d.rank, d.seq, &st)) {
                    done = false; /* acks are read in channel order */
                    continue;
                }
                tt_->p2p_send_read_[d.rank] = d.seq;
                d.acked = true;
                if (st != 0 && result_ == UCC_OK) {
                    result_ = (ucc_status_t)st;
                }
            }
        }
        if (!done) {
            return UCC_INPROGRESS;
        }
        if (tmpl_.status != 0 && result_ == UCC_OK) {
            result_ = (ucc_status_t)tmpl_.status;
        }
        return result_;
    }

    /* member: 0 wait for my descriptor and launch, 1 poll the completion
     * word, 2 ack in channel order */
    ucc_status_t step_member()
    {
        P2pMbox &mb = tt_->mbox_;
        if (phase_ == 0) {
            if (tt_->p2p_recv_taken_[root_] + 1 != seq_) {
                return UCC_INPROGRESS; /* an earlier recv goes first */
            }
            const P2pDesc *d = mb.peek(root_, me_, seq_);
            if (!d) {
                return UCC_INPROGRESS;
            }
            tt_->p2p_recv_taken_[root_] = seq_; /* consumed either way */
            const bool has_tag = a_.mask & UCC_COLL_ARGS_FIELD_TAG;
            if (d->status != 0) {
                ucc_error("active-set bcast from rank %u: the root could "
                          "not export its source", root_);
                result_ = (ucc_status_t)d->status;
            } else if (has_tag && d->has_tag && d->tag != a_.tag) {
                ucc_error("active-set bcast from rank %u: tag mismatch, "
                          "root posted %u, this rank %u", root_,
                          (unsigned)d->tag, (unsigned)a_.tag);
                result_ = UCC_ERR_INVALID_PARAM;
            } else if (d->len != bytes_) {
                ucc_error("active-set bcast from rank %u: length mismatch, "
                          "root posted %llu bytes, this rank %llu", root_,
                          (unsigned long long)d->len,
                          (unsigned long long)bytes_);
                result_ = UCC_ERR_INVALID_PARAM;
            } else {
                result_ = launch_pull(*d);
            }
            phase_ = result_ == UCC_OK ? 1 : 2;
        }
        if (phase_ == 1) {
            if (__atomic_load_n(tt_->p2p_done_host_, __ATOMIC_ACQUIRE) <
                launch_) {
                return UCC_INPROGRESS;
            }
            phase_ = 2;
        }
        if (!mb.can_ack(root_, me_, seq_)) {
            return UCC_INPROGRESS;
        }
        mb.ack(root_, me_, seq_, (int32_t)result_);
        return result_;
    }

    ucc_status_t launch_pull(const P2pDesc &d)
    {
        const uint8_t *src = nullptr;
        if (d.pid == (int32_t)getpid()) {
            src = (const uint8_t *)(uintptr_t)d.raw_ptr; /* in-process jig */
        } else if (bytes_ > 0) {
            if (!d.has_handle) {
                return UCC_ERR_NO_RESOURCE;
            }
            hipIpcMemHandle_t h;
            memcpy(&h, d.handle, sizeof(h));
            void *m =
                tt_->ipc_open_cached(d.pid, d.raw_ptr - d.base_off, h);
            if (!m) {
                ucc_error("active-set bcast from rank %u: IPC open of the "
                          "source failed", root_);
                return UCC_ERR_NO_RESOURCE;
            }
            src = (const uint8_t *)m + d.base_off;
        }
        ec_hip::P2pPullArgs pa{};
        pa.dst     = a_.src.info.buffer;
        pa.src     = src;
        pa.len     = bytes_;
        pa.nblocks = tt_->cfg_.p2p_blocks > 0
                         ? tt_->cfg_.p2p_blocks
                         : ec_hip::p2p_auto_blocks(bytes_);
        pa.arrive_cnt  = tt_->p2p_cnt_;
        pa.done_host   = tt_->p2p_done_host_;
        pa.done_target = tt_->p2p_blocks_cum_ + (uint64_t)pa.nblocks;
        pa.done_seq    = tt_->p2p_launches_ + 1;
        ucc_status_t st = ec_hip::p2p_pull(pa, comp());
        if (st != UCC_OK) {
            return st;
        }
        tt_->p2p_blocks_cum_ = pa.done_target;
        tt_->p2p_launches_   = pa.done_seq;
        launch_              = pa.done_seq;
        return UCC_OK;
    }

    size_t           bytes_ = 0;
    uint32_t         root_  = 0;
    uint64_t         seq_   = 0; /* member: my seq on channel root->me */
    uint64_t         launch_ = 0;
    ucc_status_t     result_ = UCC_OK;
    std::vector<Dst> dsts_;      /* root: one entry per other member   */
    P2pDesc          tmpl_{};
    bool             exported_ = false;
};

/* ------------------------------------------------------------ scoring  */
class Cdna4Tl final : public Tl {
  public:
    const char *name() const override { return "cdna4"; }
    int         default_score() const override { return 80; }

    TlContext *context_create(Context *ctx) override
    {
        auto &cfg = Config::instance();
        cfg.declare("TL_CDNA4", "ENABLE", "1",
                    "enable the native xGMI device transport");
        cfg.declare("TL_CDNA4", "MAX_CONCURRENT", "4",
                    "rotating in-flight collective slots");
        cfg.declare("TL_CDNA4", "PERSISTENT_SLOTS", "2",
                    "dedicated slots for persistent triggered colls");
        cfg.declare("TL_CDNA4", "CHUNK_SIZE", "32m",
                    "staging fragment bytes per slot area");
        cfg.declare("TL_CDNA4", "FUSED_MAX", "4m",
                    "max msg bytes for the fused single-kernel allreduce "
                    "(measured crossover vs the gated pipeline, "
                    "profiles/rocprof_kernels_r02.md)");
        cfg.declare("TL_CDNA4", "GATED", "1",
                    "device-gated pipeline for large colls");
        cfg.declare("TL_CDNA4", "SPIN_LIMIT", "0",
                    "device spin bound override (0 = default ~seconds)");
        cfg.declare("TL_CDNA4", "GATED_BLOCKS", "0",
                    "gated-pipeline kernel grid size (workgroups of 256; "
                    "0 = built-in default; must match on every rank). Any "
                    "value >= 1 is correct at any team size, also a grid "
                    "smaller than the team: the gather kernel's blocks "
                    "then take whole sources in turn");
        cfg.declare("TL_CDNA4", "STAGE_SDMA", "0",
                    "stage fragments with hipMemcpyAsync (SDMA) "
                    "instead of a copy kernel");
        cfg.declare("TL_CDNA4", "CE_ALLTOALL", "1",
                    "move zero-copy alltoall data on SDMA copy engines "
                    "(hipMemcpyAsync) instead of gather kernels");
        cfg.declare("TL_CDNA4", "ZC_DEFRAG", "1",
                    "single-fragment zero-copy collectives (debug off)");
        cfg.declare("TL_CDNA4", "ZC_FUSED", "1",
                    "zero-copy allreduce/reduce_scatter as one kernel "
                    "per post; 0 = stage/reduce/gather launches (debug)");
        cfg.declare("TL_CDNA4", "ZC_STREAM", "auto",
                    "non-temporal (streaming) data phase of the one-kernel "
                    "zero-copy allreduce: auto = 2 ranks from 128 MiB, "
                    "0 = never, 1 = wherever a streamed kernel exists "
                    "(depth 4), reduce_scatter and reduce included");
        cfg.declare("TL_CDNA4", "PUSH", "1",
                    "push-model gated flags; 0 = remote-poll fallback "
                    "(debug)");
        cfg.declare("TL_CDNA4", "CE_ALLTOALL_MIN", "192m",
                    "min total message bytes for the SDMA alltoall "
                    "(measured crossover vs the gather kernel, "
                    "profiles/rocprof_kernels_r02.md)");
        cfg.declare("TL_CDNA4", "P2P", "1",
                    "device active-set bcast (p2p send/recv) over the peer "
                    "mappings; 0 = device active sets are not supported "
                    "(must match on every rank)");
        cfg.declare("TL_CDNA4", "P2P_DEPTH", "8",
                    "p2p mailbox ring depth per ordered pair (power of "
                    "two <= 64; must match on every rank)");
        cfg.declare("TL_CDNA4", "P2P_BLOCKS", "0",
                    "p2p pull kernel grid size (workgroups of 256; 0 = "
                    "size-derived, profiles/p2p_active_set.md)");
        cfg.declare("TL_CDNA4", "RING", "0",
                    "offer the host-gated multi-ring (link-partitioned) "
                    "allreduce / reduce_scatter / allgather as algorithm "
                    "'ring' at score 70, below every direct algorithm: "
                    "select it with UCC_TUNE (must match on every rank)");
        cfg.declare("TL_CDNA4", "RING_NRINGS", "0",
                    "rings of the 'ring' algorithm, one per stride coprime "
                    "to the team size, at most 4 (0 = auto: "
                    "min(4, phi(n)); must match on every rank)");
        cfg.declare("TL_CDNA4", "GATED_ROOTED", "0",
                    "serve full-team device bcast and reduce with the "
                    "device-gated pipeline (algorithm 'gated_pipeline', "
                    "score 90: scatter + allgather resp. slice reduce + "
                    "gather at the root, zero-copy for persistent and "
                    "large requests) instead of staged_linear; must be "
                    "the same on every rank");
        cfg.declare("TL_CDNA4", "FUSED_COLLS", "0",
                    "serve small full-team device allgather, allgatherv, "
                    "reduce_scatter, reduce_scatterv, alltoall, alltoallv, "
                    "bcast and reduce with one fused kernel per rank "
                    "(algorithm 'fused', score 100; stage, handshake, read "
                    "over the peer mappings, hipGraph-replayable but for "
                    "alltoallv, whose ranks vote in the kernel whether "
                    "every pair fits and else fall back together); must be "
                    "the same on every rank");
        cfg.declare("TL_CDNA4", "FUSED_COLLS_MAX", "8k",
                    "max scratch bytes of one fused collective (the "
                    "per-rank block of allgather, n blocks of "
                    "reduce_scatter and alltoall, the vector of bcast and "
                    "reduce, blocks rounded up to 16; allgatherv: the "
                    "largest block; reduce_scatterv: the sum of the "
                    "blocks; alltoallv: a 16-byte header and n cells, so "
                    "the largest fused pair is (MAX - 16) / n rounded down "
                    "to 16); capped at "
                    "CHUNK_SIZE. Default: the largest size at which "
                    "fused beat every other path of all five types, "
                    "persistent zero-copy reduce_scatter included; "
                    "one-shot requests gain up to 1m "
                    "(profiles/fused_colls.md)");
        cfg.declare("TL_CDNA4", "FUSED_GATHER_SCATTER", "0",
                    "serve small full-team device gather, scatter, gatherv "
                    "and scatterv with one fused kernel per rank (algorithm "
                    "'fused', score 100), independently of FUSED_COLLS and "
                    "within FUSED_COLLS_MAX: gather takes the per-rank "
                    "block, scatter n blocks, each rounded up to 16. "
                    "gatherv and scatterv, whose counts only the root "
                    "knows, take a 144-byte header off the bound, "
                    "B = MAX - 144 rounded down to 16; the root decides "
                    "inside the kernel: gatherv fits if the largest block "
                    "is at most B, scatterv if the sum of the blocks, each "
                    "rounded up to 16, is at most B; otherwise all ranks "
                    "fall back together to staged_linear. gather and "
                    "scatter are hipGraph-replayable; must be the same on "
                    "every rank");
        if (!cfg.get_bool("TL_CDNA4", "ENABLE", true) ||
            !mc::hip_available()) {
            return nullptr;
        }
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) {
            return nullptr;
        }
        ctx->proc.device = dev;
        return new Cdna4TlContext(ctx, this, dev);
    }

    TlTeam *team_create(TlContext *tlc, Team *team) override
    {
        if (team->size < 2 || team->size > (uint32_t)kMaxRanks ||
            !team->all_same_node() || !team->all_have_device()) {
            return nullptr;
        }
        auto    &cfg = Config::instance();
        Cdna4Cfg c;
        c.nslots    = (uint32_t)cfg.get_int("TL_CDNA4", "MAX_CONCURRENT", 4);
        c.npers  = (uint32_t)cfg.get_int("TL_CDNA4", "PERSISTENT_SLOTS", 2);
        if (c.nslots + c.npers > 8) { /* flags layout: 8 slots max */
            c.npers = c.nslots < 8 ? 8 - c.nslots : 0;
        }
        c.chunk     = cfg.get_size("TL_CDNA4", "CHUNK_SIZE", 32 * 1024 * 1024);
        c.spin_limit =
            (uint64_t)cfg.get_int("TL_CDNA4", "SPIN_LIMIT", 0);
        c.fused_max = cfg.get_size("TL_CDNA4", "FUSED_MAX",
                                   4 * 1024 * 1024);
        {
            const std::string zs = cfg.get("TL_CDNA4", "ZC_STREAM", "auto");
            c.zc_stream = zs == "0"   ? tl_cdna4::ZC_STREAM_OFF
                          : zs == "1" ? tl_cdna4::ZC_STREAM_ON
                                      : tl_cdna4::ZC_STREAM_AUTO;
        }
        c.gated_blocks =
            (int)cfg.get_int("TL_CDNA4", "GATED_BLOCKS", 0);
        if (c.gated_blocks < 0) {
            c.gated_blocks = 0;
        }
        if (c.gated_blocks > ec_hip::kGatedMaxBlocks) {
            c.gated_blocks = ec_hip::kGatedMaxBlocks;
        }
        c.ce_alltoall = cfg.get_bool("TL_CDNA4", "CE_ALLTOALL", true);
        c.ce_alltoall_min =
            cfg.get_size("TL_CDNA4", "CE_ALLTOALL_MIN",
                         192 * 1024 * 1024);
        c.p2p       = cfg.get_bool("TL_CDNA4", "P2P", true);
        c.p2p_depth = p2p_clamp_depth(
            (long)cfg.get_int("TL_CDNA4", "P2P_DEPTH", 8));
        c.p2p_blocks = (int)cfg.get_int("TL_CDNA4", "P2P_BLOCKS", 0);
        if (c.p2p_blocks < 0) {
            c.p2p_blocks = 0;
        }
        if (c.p2p_blocks > ec_hip::kP2pMaxBlocks) {
            c.p2p_blocks = ec_hip::kP2pMaxBlocks;
        }
        c.gated_rooted = cfg.get_bool("TL_CDNA4", "GATED_ROOTED", false);
        c.ring        = cfg.get_bool("TL_CDNA4", "RING", false);
        c.ring_nrings = (int)cfg.get_int("TL_CDNA4", "RING_NRINGS", 0);
        if (c.ring_nrings < 0) {
            c.ring_nrings = 0;
        }
        if (c.ring_nrings > kRingMaxRings) {
            c.ring_nrings = kRingMaxRings;
        }
        c.fused_colls = cfg.get_bool("TL_CDNA4", "FUSED_COLLS", false);
        c.fused_colls_max =
            cfg.get_size("TL_CDNA4", "FUSED_COLLS_MAX", 8 * 1024);
        c.fused_gather_scatter =
            cfg.get_bool("TL_CDNA4", "FUSED_GATHER_SCATTER", false);
        return new Cdna4TlTeam(tlc, team, c);
    }
};

static Cdna4Tl g_cdna4_tl;

Tl *Cdna4TlContext::iface() { return &g_cdna4_tl; }

/* alltoall(v) in place has no staged or gated form: refused when the
 * request is initialised, not when it is posted */
static bool inplace_alltoall(const ucc_coll_args_t &args)
{
    return (args.coll_type == UCC_COLL_TYPE_ALLTOALL ||
            args.coll_type == UCC_COLL_TYPE_ALLTOALLV) &&
           (args.flags & UCC_COLL_ARGS_FLAG_IN_PLACE);
}

ucc_status_t Cdna4TlTeam::init_gated(const ucc_coll_args_t &args, Team *t,
                                     Task **task)
{
    if (args.mask & UCC_COLL_ARGS_FIELD_ACTIVE_SET) {
        return UCC_ERR_NOT_SUPPORTED; /* active_set_p2p only */
    }
    if (inplace_alltoall(args)) {
        return UCC_ERR_NOT_SUPPORTED;
    }
    if (args.coll_type == UCC_COLL_TYPE_ALLREDUCE ||
        args.coll_type == UCC_COLL_TYPE_REDUCE_SCATTER ||
        args.coll_type == UCC_COLL_TYPE_REDUCE_SCATTERV) {
        ucc_datatype_t gdt = args.coll_type == UCC_COLL_TYPE_REDUCE_SCATTERV
                                 ? args.dst.info_v.datatype
                                 : args.dst.info.datatype;
        if (!ec_hip::op_supported(gdt, args.op)) {
            return UCC_ERR_NOT_SUPPORTED;
        }
    }
    if (args.coll_type == UCC_COLL_TYPE_REDUCE &&
        !ec_hip::op_supported(args.src.info.datatype, args.op)) {
        return UCC_ERR_NOT_SUPPORTED;
    }
    /* in-process multi-rank jigs can serialize spinning kernels on one HW
     * queue: host-gated staged path is the safe fallback there (same
     * reasoning as the fused kernel). */
    int same_proc = 0;
    for (auto &p : t->procs) {
        same_proc += (p.pid == t->ctx->proc.pid);
    }
    if (same_proc > 1) {
        return UCC_ERR_NOT_SUPPORTED;
    }
    *task = new GatedCollTask(t->ctx, this, args);
    return UCC_OK;
}

ucc_status_t Cdna4TlTeam::init_staged(const ucc_coll_args_t &args, Team *t,
                                      bool fused, Task **task)
{
    /* subset colls never take the team-wide slot sequence: non-members
     * post nothing (active_set_p2p serves bcast) */
    if (args.mask & UCC_COLL_ARGS_FIELD_ACTIVE_SET) {
        return UCC_ERR_NOT_SUPPORTED;
    }
    if (inplace_alltoall(args)) {
        return UCC_ERR_NOT_SUPPORTED;
    }
    /* reductions need a supported dtype x op on device */
    if (args.coll_type == UCC_COLL_TYPE_ALLREDUCE ||
        args.coll_type == UCC_COLL_TYPE_REDUCE ||
        args.coll_type == UCC_COLL_TYPE_REDUCE_SCATTER ||
        args.coll_type == UCC_COLL_TYPE_REDUCE_SCATTERV) {
        ucc_datatype_t dt = args.coll_type == UCC_COLL_TYPE_REDUCE_SCATTERV
                                ? args.dst.info_v.datatype
                                : args.dst.info.datatype;
        if (args.coll_type == UCC_COLL_TYPE_REDUCE) {
            dt = args.src.info.datatype;
        }
        if (!ec_hip::op_supported(dt, args.op)) {
            return UCC_ERR_NOT_SUPPORTED;
        }
    }
    if (fused) {
        /* The fused kernel spin-waits for every peer's kernel. With
         * several ranks of one process on one GPU (the in-process jig)
         * their streams can share a HW queue and event barrier packets
         * serialize the dispatches -> deadlock. One process per GPU
         * (production) is safe; same-process multi-rank falls back to the
         * host-gated staged path. */
        int same_proc = 0;
        for (auto &p : t->procs) {
            same_proc += (p.pid == t->ctx->proc.pid);
        }
        if (same_proc > 1) {
            return UCC_ERR_NOT_SUPPORTED;
        }
        *task = new FusedAllreduceTask(t->ctx, this, args);
    } else {
        *task = new StagedTask(t->ctx, this, args);
    }
    return UCC_OK;
}

ucc_status_t Cdna4TlTeam::init_unfused(const ucc_coll_args_t &args, Team *t,
                                       Task **task, const char **alg)
{
    /* get_scores() below registers gated_pipeline for the v-forms exactly
     * when GATED is set, and never for gatherv and scatterv */
    const bool rooted_v = args.coll_type == UCC_COLL_TYPE_GATHERV ||
                          args.coll_type == UCC_COLL_TYPE_SCATTERV;
    if (!rooted_v && Config::instance().get_bool("TL_CDNA4", "GATED", true) &&
        init_gated(args, t, task) == UCC_OK) {
        *alg = "gated_pipeline";
        return UCC_OK;
    }
    *alg = "staged_linear";
    return init_staged(args, t, false, task);
}

void Cdna4TlTeam::get_scores(Team *team, ScoreMap &map)
{
    (void)team;
    Cdna4TlTeam *self = this;
    auto add_gated = [&](ucc_coll_type_t ct, size_t lo, size_t hi,
                         int score) {
        ScoreRange r;
        r.start    = lo;
        r.end      = hi;
        r.score    = score;
        r.tl_name  = "cdna4";
        r.alg_name = "gated_pipeline";
        r.init     = [self](const ucc_coll_args_t &args, Team *t,
                        Task **task) -> ucc_status_t {
            return self->init_gated(args, t, task);
        };
        for (auto mt : {UCC_MEMORY_TYPE_CUDA, UCC_MEMORY_TYPE_CUDA_MANAGED}) {
            map.add(ct, mt, r);
        }
    };
    auto add = [&](ucc_coll_type_t ct, size_t lo, size_t hi, int score,
                   const char *alg, bool fused) {
        ScoreRange r;
        r.start    = lo;
        r.end      = hi;
        r.score    = score;
        r.tl_name  = "cdna4";
        r.alg_name = alg;
        r.init     = [self, fused](const ucc_coll_args_t &args, Team *t,
                               Task **task) -> ucc_status_t {
            return self->init_staged(args, t, fused, task);
        };
        for (auto mt : {UCC_MEMORY_TYPE_CUDA, UCC_MEMORY_TYPE_CUDA_MANAGED}) {
            map.add(ct, mt, r);
        }
    };
    if (cfg_.p2p) {
        ScoreRange r;
        r.start    = 0;
        r.end      = SIZE_MAX;
        r.score    = 95;
        r.tl_name  = "cdna4";
        r.alg_name = "active_set_p2p";
        r.init     = [self](const ucc_coll_args_t &args, Team *t,
                        Task **task) -> ucc_status_t {
            if (!(args.mask & UCC_COLL_ARGS_FIELD_ACTIVE_SET)) {
                return UCC_ERR_NOT_SUPPORTED;
            }
            /* packed (non-contiguous generic) datatypes need a host
             * pack/unpack pass: not on this path */
            const ucc_datatype_t dt = args.src.info.datatype;
            if (!ucc_dt_is_predefined(dt)) {
                const ucc_generic_dt_ops_t *g = ucc_dt_generic_ops(dt);
                if (!g || !(g->flags & UCC_GENERIC_DT_OPS_FLAG_CONTIG)) {
                    return UCC_ERR_NOT_SUPPORTED;
                }
            }
            *task = new ActiveSetBcastTask(t->ctx, self, args);
            return UCC_OK;
        };
        map.add(UCC_COLL_TYPE_BCAST, UCC_MEMORY_TYPE_CUDA, r);
    }
    /* the score-100 entry of the fused one-kernel collectives, for the
     * types a knob switches on: the task class follows the type, the
     * declines are the same for all of them */
    auto add_fused = [&](std::initializer_list<ucc_coll_type_t> types) {
        ScoreRange r;
        r.start    = 0;
        r.end      = SIZE_MAX;
        r.score    = 100;
        r.tl_name  = "cdna4";
        r.alg_name = "fused";
        r.init     = [self](const ucc_coll_args_t &args, Team *t,
                        Task **task) -> ucc_status_t {
            const bool a2av = args.coll_type == UCC_COLL_TYPE_ALLTOALLV;
            const bool rooted_v =
                args.coll_type == UCC_COLL_TYPE_GATHERV ||
                args.coll_type == UCC_COLL_TYPE_SCATTERV;
            if ((args.mask & UCC_COLL_ARGS_FIELD_ACTIVE_SET) ||
                !(a2av       ? FusedA2avTask::supported(args, self)
                  : rooted_v ? FusedRootedVTask::supported(args, self)
                             : FusedCollTask::supported(args, self))) {
                return UCC_ERR_NOT_SUPPORTED;
            }
            /* spinning kernels of several ranks of one process can share
             * a HW queue: see the fused allreduce below */
            int same_proc = 0;
            for (auto &p : t->procs) {
                same_proc += (p.pid == t->ctx->proc.pid);
            }
            if (same_proc > 1) {
                return UCC_ERR_NOT_SUPPORTED;
            }
            if (a2av) {
                *task = new FusedA2avTask(t->ctx, self, args);
            } else if (rooted_v) {
                *task = new FusedRootedVTask(t->ctx, self, args);
            } else {
                *task = new FusedCollTask(t->ctx, self, args);
            }
            return UCC_OK;
        };
        for (auto ct : types) {
            for (auto mt :
                 {UCC_MEMORY_TYPE_CUDA, UCC_MEMORY_TYPE_CUDA_MANAGED}) {
                map.add(ct, mt, r);
            }
        }
    };
    if (cfg_.fused_colls) {
        /* opt-in (UCC_TL_CDNA4_FUSED_COLLS): unset, the map is exactly the
         * entries below. A declined request (over the bound, in-place
         * alltoall, ...) falls through to them. */
        add_fused({UCC_COLL_TYPE_ALLGATHER, UCC_COLL_TYPE_REDUCE_SCATTER,
                   UCC_COLL_TYPE_ALLTOALL, UCC_COLL_TYPE_BCAST,
                   UCC_COLL_TYPE_REDUCE, UCC_COLL_TYPE_ALLGATHERV,
                   UCC_COLL_TYPE_REDUCE_SCATTERV, UCC_COLL_TYPE_ALLTOALLV});
    }
    if (cfg_.fused_gather_scatter) {
        /* opt-in of its own (UCC_TL_CDNA4_FUSED_GATHER_SCATTER), whatever
         * FUSED_COLLS says: unset, the four types keep staged_linear */
        add_fused({UCC_COLL_TYPE_GATHER, UCC_COLL_TYPE_SCATTER,
                   UCC_COLL_TYPE_GATHERV, UCC_COLL_TYPE_SCATTERV});
    }
    add(UCC_COLL_TYPE_ALLREDUCE, 0, cfg_.fused_max, 100, "fused", true);
    if (Config::instance().get_bool("TL_CDNA4", "GATED", true)) {
        add_gated(UCC_COLL_TYPE_ALLREDUCE, cfg_.fused_max + 1, SIZE_MAX,
                  90);
        add_gated(UCC_COLL_TYPE_REDUCE_SCATTER, 0, SIZE_MAX, 90);
        add_gated(UCC_COLL_TYPE_REDUCE_SCATTERV, 0, SIZE_MAX, 90);
        add_gated(UCC_COLL_TYPE_ALLGATHER, 0, SIZE_MAX, 90);
        add_gated(UCC_COLL_TYPE_ALLGATHERV, 0, SIZE_MAX, 90);
        add_gated(UCC_COLL_TYPE_ALLTOALL, 0, SIZE_MAX, 90);
        add_gated(UCC_COLL_TYPE_ALLTOALLV, 0, SIZE_MAX, 90);
        if (cfg_.gated_rooted) {
            /* opt-in (UCC_TL_CDNA4_GATED_ROOTED): unset, bcast and reduce
             * keep exactly the staged_linear entries below */
            add_gated(UCC_COLL_TYPE_BCAST, 0, SIZE_MAX, 90);
            add_gated(UCC_COLL_TYPE_REDUCE, 0, SIZE_MAX, 90);
        }
    }
    add(UCC_COLL_TYPE_ALLREDUCE, 0, SIZE_MAX, 80, "staged_linear", false);
    add(UCC_COLL_TYPE_ALLGATHER, 0, SIZE_MAX, 80, "staged_linear", false);
    add(UCC_COLL_TYPE_ALLGATHERV, 0, SIZE_MAX, 80, "staged_linear", false);
    add(UCC_COLL_TYPE_REDUCE_SCATTER, 0, SIZE_MAX, 80, "staged_linear",
        false);
    add(UCC_COLL_TYPE_REDUCE_SCATTERV, 0, SIZE_MAX, 80, "staged_linear",
        false);
    add(UCC_COLL_TYPE_BCAST, 0, SIZE_MAX, 80, "staged_linear", false);
    add(UCC_COLL_TYPE_REDUCE, 0, SIZE_MAX, 80, "staged_linear", false);
    add(UCC_COLL_TYPE_ALLTOALL, 0, SIZE_MAX, 80, "staged_linear", false);
    add(UCC_COLL_TYPE_ALLTOALLV, 0, SIZE_MAX, 80, "staged_linear", false);
    add(UCC_COLL_TYPE_GATHER, 0, SIZE_MAX, 80, "staged_linear", false);
    add(UCC_COLL_TYPE_GATHERV, 0, SIZE_MAX, 80, "staged_linear", false);
    add(UCC_COLL_TYPE_SCATTER, 0, SIZE_MAX, 80, "staged_linear", false);
    add(UCC_COLL_TYPE_SCATTERV, 0, SIZE_MAX, 80, "staged_linear", false);
    if (cfg_.ring) {
        /* opt-in, and even then below every direct algorithm until
         * UCC_TUNE lifts it */
        ScoreRange r;
        r.start    = 0;
        r.end      = SIZE_MAX;
        r.score    = 70;
        r.tl_name  = "cdna4";
        r.alg_name = "ring";
        r.init     = [self](const ucc_coll_args_t &args, Team *t,
                        Task **task) -> ucc_status_t {
            if ((args.mask & UCC_COLL_ARGS_FIELD_ACTIVE_SET) ||
                !RingTask::supported(args, self)) {
                return UCC_ERR_NOT_SUPPORTED;
            }
            *task = new RingTask(t->ctx, self, args);
            return UCC_OK;
        };
        for (auto ct : {UCC_COLL_TYPE_ALLREDUCE, UCC_COLL_TYPE_REDUCE_SCATTER,
                        UCC_COLL_TYPE_ALLGATHER}) {
            for (auto mt :
                 {UCC_MEMORY_TYPE_CUDA, UCC_MEMORY_TYPE_CUDA_MANAGED}) {
                map.add(ct, mt, r);
            }
        }
    }
}

} // namespace

Tl *tl_cdna4_iface() { return &g_cdna4_tl; }

} // namespace ucc
