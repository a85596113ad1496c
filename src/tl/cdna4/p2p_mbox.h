/* Per-pair mailbox segment: the control channel of tl/cdna4's device
 * active-set bcast (p2p send/recv over the peer mappings).
 *
 * The slot segment (slot_seg.h) assumes that every rank of the team posts
 * every collective in the same order. A subset transfer breaks that, so
 * it gets a channel of its own per ORDERED pair (root -> member), n x n
 * channels in one small POSIX-shm segment. Rank 0 creates it, the others
 * attach, exactly like the slot segment.
 *
 * One channel:
 *   line 0   posted   monotone, written by the root (release)
 *   line 1   acked    monotone, written by the member (release)
 *   line 2+  ack status per ring slot, written by the member before acked
 *   then     ring of D descriptors, written by the root before posted
 *
 * Sequence numbers start at 1. Descriptor s lives in ring slot
 * (s - 1) & (D - 1); the root may write it once s - acked <= D. Both
 * counters move by exactly one per transfer, in order: transfers on one
 * pair match in post order (non-overtaking), different pairs are
 * independent.
 *
 * Pure host code, no HIP calls: tests/native/test_p2p_mbox.cc runs it
 * without a GPU and under the host sanitizers. */
#ifndef UCC_AMD_P2P_MBOX_H_
#define UCC_AMD_P2P_MBOX_H_

#include <atomic>
#include <cstring>
#include <string>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../api/ucc.h"

namespace ucc {

constexpr uint32_t kP2pMagic    = 0x55cc9292;
constexpr uint32_t kP2pMaxDepth = 64;
constexpr size_t   kP2pLine     = 64;

/* what the root tells one member about one transfer */
struct P2pDesc {
    uint64_t seq;      /* sequence number on this channel              */
    uint64_t len;      /* bytes                                        */
    uint64_t raw_ptr;  /* source pointer in the exporter's VA space    */
    uint64_t base_off; /* raw_ptr - base of its allocation             */
    int32_t  pid;      /* exporter                                     */
    int32_t  status;   /* 0, or the root's error (export failed)       */
    uint16_t tag;
    uint16_t has_tag;
    uint32_t has_handle; /* 0: same-process peers only, handle unset   */
    uint8_t  handle[64]; /* hipIpcMemHandle_t of the allocation        */
};
static_assert(sizeof(P2pDesc) == 112, "P2pDesc layout");

/* ring depth knob -> power of two in [1, kP2pMaxDepth] (rounds down) */
static inline uint32_t p2p_clamp_depth(long v)
{
    if (v < 1) {
        v = 1;
    }
    if (v > (long)kP2pMaxDepth) {
        v = kP2pMaxDepth;
    }
    uint32_t d = 1;
    while (d * 2 <= (uint32_t)v) {
        d *= 2;
    }
    return d;
}

class P2pMbox {
  public:
    ucc_status_t create(const std::string &name, uint32_t nranks,
                        uint32_t depth)
    {
        name_  = name;
        owner_ = true;
        set_geom(nranks, depth);
        shm_unlink(name.c_str()); /* stale cleanup */
        int fd = shm_open(name.c_str(), O_CREAT | O_EXCL | O_RDWR, 0600);
        if (fd < 0) {
            return UCC_ERR_NO_RESOURCE;
        }
        if (ftruncate(fd, (off_t)size_) != 0) {
            close(fd);
            shm_unlink(name.c_str());
            return UCC_ERR_NO_MEMORY;
        }
        base_ = mmap(nullptr, size_, PROT_READ | PROT_WRITE, MAP_SHARED, fd,
                     0);
        close(fd);
        if (base_ == MAP_FAILED) {
            base_ = nullptr;
            shm_unlink(name.c_str());
            return UCC_ERR_NO_MEMORY;
        }
        /* fresh shm pages are zero: every counter starts at 0 */
        auto *h   = (Header *)base_;
        h->nranks = nranks;
        h->depth  = depth;
        ((std::atomic<uint32_t> *)&h->magic)
            ->store(kP2pMagic, std::memory_order_release);
        return UCC_OK;
    }

    /* UCC_INPROGRESS while the creator has not made the segment yet */
    ucc_status_t attach(const std::string &name, uint32_t nranks,
                        uint32_t depth)
    {
        name_  = name;
        owner_ = false;
        set_geom(nranks, depth);
        int fd = shm_open(name.c_str(), O_RDWR, 0600);
        if (fd < 0) {
            return UCC_INPROGRESS;
        }
        struct stat st;
        if (fstat(fd, &st) != 0 || (size_t)st.st_size < size_) {
            close(fd);
            return UCC_INPROGRESS;
        }
        base_ = mmap(nullptr, size_, PROT_READ | PROT_WRITE, MAP_SHARED, fd,
                     0);
        close(fd);
        if (base_ == MAP_FAILED) {
            base_ = nullptr;
            return UCC_ERR_NO_MEMORY;
        }
        return UCC_OK;
    }

    bool attached() const { return base_ != nullptr; }

    bool ready() const
    {
        if (!base_) {
            return false;
        }
        auto *h = (const Header *)base_;
        return ((const std::atomic<uint32_t> *)&h->magic)
                   ->load(std::memory_order_acquire) == kP2pMagic;
    }

    ~P2pMbox()
    {
        if (base_) {
            munmap(base_, size_);
        }
        if (owner_) {
            shm_unlink(name_.c_str());
        }
    }

    uint32_t depth() const { return depth_; }

    /* ---- both sides */
    uint64_t posted(uint32_t root, uint32_t member) const
    {
        return ctr(root, member, 0)->load(std::memory_order_acquire);
    }
    uint64_t acked(uint32_t root, uint32_t member) const
    {
        return ctr(root, member, 1)->load(std::memory_order_acquire);
    }

    /* ---- root side */
    /* may descriptor `seq` be written now? In order, and its ring slot
     * must have been acked (seq - acked <= D) */
    bool can_post(uint32_t root, uint32_t member, uint64_t seq) const
    {
        return posted(root, member) + 1 == seq &&
               seq - acked(root, member) <= depth_;
    }
    void post(uint32_t root, uint32_t member, const P2pDesc &d)
    {
        memcpy(slot(root, member, d.seq), &d, sizeof(d));
        ctr(root, member, 0)->store(d.seq, std::memory_order_release);
    }
    /* has the member acked `seq`? *status gets what it reported. The
     * status slot is reused by seq + D, which the root can only post
     * after this ack: read it before posting further. */
    bool ack_of(uint32_t root, uint32_t member, uint64_t seq,
                int32_t *status) const
    {
        if (acked(root, member) < seq) {
            return false;
        }
        *status = ack_status(root, member, seq)
                      ->load(std::memory_order_relaxed);
        return true;
    }

    /* ---- member side */
    /* descriptor `seq` once the root has posted it, else nullptr */
    const P2pDesc *peek(uint32_t root, uint32_t member, uint64_t seq) const
    {
        if (posted(root, member) < seq) {
            return nullptr;
        }
        return slot(root, member, seq);
    }
    /* in order only: the caller acks seq after seq - 1 */
    bool can_ack(uint32_t root, uint32_t member, uint64_t seq) const
    {
        return acked(root, member) + 1 == seq;
    }
    void ack(uint32_t root, uint32_t member, uint64_t seq, int32_t status)
    {
        ack_status(root, member, seq)
            ->store(status, std::memory_order_relaxed);
        ctr(root, member, 1)->store(seq, std::memory_order_release);
    }

  private:
    struct Header {
        uint32_t magic;
        uint32_t nranks;
        uint32_t depth;
    };
    void set_geom(uint32_t nranks, uint32_t depth)
    {
        nranks_ = nranks;
        depth_  = depth;
        /* posted line, acked line, D status words, D descriptors */
        size_t st = ((size_t)depth * sizeof(int32_t) + kP2pLine - 1) /
                    kP2pLine * kP2pLine;
        ring_off_ = 2 * kP2pLine + st;
        chan_sz_  = (ring_off_ + (size_t)depth * sizeof(P2pDesc) +
                    kP2pLine - 1) /
                   kP2pLine * kP2pLine;
        size_ = kP2pLine + (size_t)nranks * nranks * chan_sz_;
    }
    uint8_t *chan(uint32_t root, uint32_t member) const
    {
        return (uint8_t *)base_ + kP2pLine +
               ((size_t)root * nranks_ + member) * chan_sz_;
    }
    std::atomic<uint64_t> *ctr(uint32_t root, uint32_t member,
                               int which) const
    {
        return (std::atomic<uint64_t> *)(chan(root, member) +
                                         (size_t)which * kP2pLine);
    }
    std::atomic<int32_t> *ack_status(uint32_t root, uint32_t member,
                                     uint64_t seq) const
    {
        return (std::atomic<int32_t> *)(chan(root, member) + 2 * kP2pLine) +
               ((seq - 1) & (depth_ - 1));
    }
    P2pDesc *slot(uint32_t root, uint32_t member, uint64_t seq) const
    {
        return (P2pDesc *)(chan(root, member) + ring_off_) +
               ((seq - 1) & (depth_ - 1));
    }

    void       *base_  = nullptr;
    size_t      size_  = 0;
    bool        owner_ = false;
    std::string name_;
    uint32_t    nranks_ = 0, depth_ = 0;
    size_t      ring_off_ = 0, chan_sz_ = 0;
};

} // namespace ucc

#endif
