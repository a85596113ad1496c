"""Worker for tests/test_p2p_gpu.py: tl/cdna4's device active-set bcast
(p2p send/recv), run once under
  python -m torch.distributed.run --standalone --nnodes=1 \
      --nproc-per-node=N tests/p2p_worker.py MODE

MODE four     4 ranks: single pair with idle ranks, both directions, ring
              with back-pressure, three active sets, persistent re-post,
              interleaving with team-wide collectives, tag / length
              mismatch
MODE two      2 ranks: PipelineStage on CUDA bf16 tensors
MODE two_off  the same with UCC_TL_CDNA4_P2P=0 (host fallback)
MODE --bench  2 ranks: PipelineEdge round trips, one JSON line
MODE --sweep  1 process: pull-kernel block-count sweep, one JSON line

All ranks share cuda:0. Every payload is seeded, so every rank knows what
every other rank sends and checks what it received byte for byte. Every
request carries timeout=30: a protocol bug ends as UCC_ERR_TIMED_OUT from
the progress queue, never as a stuck process. Wait loops poll all
outstanding requests and drive ctx.progress().
"""

import json
import os
import sys
import time

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ucc_amd import core, dtypes  # noqa: E402
from ucc_amd.parallel import Communicator  # noqa: E402
from ucc_amd.parallel.pp import PipelineEdge, PipelineStage  # noqa: E402

TIMEOUT = 30
MiB = 1 << 20


def payload(seed, nbytes):
    """nbytes seeded bytes (CPU uint8), equal on every rank."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (nbytes,), generator=g, dtype=torch.uint8)


class P2p:
    def __init__(self):
        torch.cuda.set_device(0)
        self.rank = int(os.environ["RANK"])
        self.world = int(os.environ["WORLD_SIZE"])
        dist.init_process_group("gloo", rank=self.rank,
                                world_size=self.world)
        self.comm = Communicator()
        self.c = self.comm.c
        self.n_p2p = 0     # active-set requests initialised here
        self.n_bcast = 0   # team-wide device bcasts initialised here

    def init(self, buf, root, aset, tag=-1, flags=0, dt=dtypes.UINT8,
             count=None):
        """One device active-set bcast request on `buf` (a CUDA tensor)."""
        self.n_p2p += 1
        return self.c.coll_init(
            self.comm.team, "bcast", src=buf.data_ptr(), dst=0,
            count=buf.numel() if count is None else count, dt=dt,
            root=root, mem_type=dtypes.MEM_CUDA, active_set=aset, tag=tag,
            flags=flags, timeout=TIMEOUT)

    def send(self, buf, dst, **kw):
        return self.init(buf, self.rank, (self.rank, dst - self.rank, 2),
                         **kw)

    def recv(self, buf, src, **kw):
        return self.init(buf, src, (src, self.rank - src, 2), **kw)

    def run(self, reqs):
        """Post all, then wait on all; returns the final statuses. An
        error that already shows at post counts as that request's status."""
        st = [None] * len(reqs)
        for i, r in enumerate(reqs):
            try:
                r.post()
            except RuntimeError:
                st[i] = r.test() if r.test() < 0 else -1
        while True:
            busy = False
            for i, r in enumerate(reqs):
                if st[i] is None:
                    s = r.test()
                    if s == self.c.INPROGRESS:
                        busy = True
                    else:
                        st[i] = s
            if not busy:
                return st
            self.comm.ctx.progress()

    def ok(self, reqs):
        st = self.run(reqs)
        assert all(s == self.c.OK for s in st), (self.rank, st)

    def finish(self, tag):
        torch.cuda.synchronize()
        dist.barrier()
        print(f"{tag} rank={self.rank} n_p2p={self.n_p2p} "
              f"n_bcast={self.n_bcast}", flush=True)
        dist.destroy_process_group()


def expect(buf, exp, what):
    torch.cuda.synchronize()
    got = buf.cpu()
    if got.dtype != torch.uint8:
        got = got.view(torch.uint8)
    assert torch.equal(got, exp), what


# ------------------------------------------------------------ four ranks
def single_pair(j):
    """1 -> 2 while ranks 0 and 3 post nothing."""
    r = j.rank
    if r not in (1, 2):
        return
    # 8 B
    src = payload(11, 8)
    buf = src.cuda() if r == 1 else torch.zeros(8, dtype=torch.uint8,
                                                device="cuda")
    j.ok([j.send(buf, 2) if r == 1 else j.recv(buf, 1)])
    expect(buf, src, "pair 8B")
    # 100 003 B, source view offset by 1 byte, destination by 5
    n = 100_003
    src = payload(12, n)
    if r == 1:
        full = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")
        view = full[1:]
        view.copy_(src)
        torch.cuda.synchronize()
        j.ok([j.send(view, 2)])
    else:
        full = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        view = full[5:5 + n]
        j.ok([j.recv(view, 1)])
        expect(view, src, "pair unaligned")
        got = full.cpu()
        assert bool((got[:5] == 0xA5).all()) and \
            bool((got[5 + n:] == 0xA5).all()), "pair unaligned: guards"
    # 8 MiB + 16 B of bf16
    n = 8 * MiB + 16
    src = payload(13, n)
    if r == 1:
        buf = src.cuda().view(torch.bfloat16)
        torch.cuda.synchronize()
        j.ok([j.send(buf, 2, dt=dtypes.BFLOAT16)])
    else:
        buf = torch.zeros(n // 2, dtype=torch.bfloat16, device="cuda")
        j.ok([j.recv(buf, 1, dt=dtypes.BFLOAT16)])
        expect(buf, src, "pair 8MiB bf16")


def both_directions(j):
    """r posts send-to and recv-from its partner before waiting on either
    (pairs 0<->1 and 2<->3)."""
    r, p = j.rank, j.rank ^ 1
    n = 64 * 1024 + 3
    out = payload(20 + r, n).cuda()
    inn = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    j.ok([j.send(out, p), j.recv(inn, p)])
    expect(inn, payload(20 + p, n), "both directions")


def ring(j):
    """12 sends to (r+1)%4 and 12 recvs from (r-1)%4, all posted before
    any wait: ring depth 8 forces back-pressure, payloads show order."""
    r, w = j.rank, j.world
    nxt, prv = (r + 1) % w, (r - 1) % w
    n, k = 4096, 12
    outs = [payload(1000 + 100 * r + i, n).cuda() for i in range(k)]
    ins = [torch.zeros(n, dtype=torch.uint8, device="cuda")
           for _ in range(k)]
    torch.cuda.synchronize()
    reqs = [j.send(outs[i], nxt, tag=i) for i in range(k)]
    reqs += [j.recv(ins[i], prv, tag=i) for i in range(k)]
    j.ok(reqs)
    for i in range(k):
        expect(ins[i], payload(1000 + 100 * prv + i, n), f"ring {i}")


def active_sets(j):
    """{1,1,3} root 2 (rank 0 idle), {0,2,2} root 2, {3,-1,2} root 3."""
    n = 70_001
    for idx, (aset, root, members) in enumerate([
            ((1, 1, 3), 2, (1, 2, 3)),
            ((0, 2, 2), 2, (0, 2)),
            ((3, -1, 2), 3, (3, 2))]):
        if j.rank not in members:
            continue
        src = payload(30 + idx, n)
        buf = src.cuda() if j.rank == root else \
            torch.zeros(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        j.ok([j.init(buf, root, aset)])
        expect(buf, src, f"active set {aset}")


def persistent(j):
    """One persistent request 0 -> 3 posted 5 times, source rewritten."""
    if j.rank not in (0, 3):
        return
    n = 33_333
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda")
    kw = dict(flags=j.c.FLAG_PERSISTENT)
    req = j.send(buf, 3, **kw) if j.rank == 0 else j.recv(buf, 0, **kw)
    for it in range(5):
        src = payload(40 + it, n)
        if j.rank == 0:
            buf.copy_(src)
            torch.cuda.synchronize()  # host-post semantics
        j.ok([req])
        if j.rank == 3:
            expect(buf, src, f"persistent {it}")


def interleave(j):
    """p2p, then a fused allreduce, a staged_linear bcast and a persistent
    gated allgather on the whole team, then p2p again: the subset
    transfers take nothing from the team-wide sequence."""
    r, w, c = j.rank, j.world, j.c
    team, ctx = j.comm.team, j.comm.ctx
    n = 50_000

    def pair(a, b, seed):
        if r not in (a, b):
            return
        src = payload(seed, n)
        buf = src.cuda() if r == a else \
            torch.zeros(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        j.ok([j.send(buf, b) if r == a else j.recv(buf, a)])
        expect(buf, src, f"interleave pair {a}->{b}")

    ag_src = torch.zeros(2048, dtype=torch.float32, device="cuda")
    ag_dst = torch.zeros(2048 * w, dtype=torch.float32, device="cuda")
    ag = c.coll_init(team, "allgather", src=ag_src.data_ptr(),
                     dst=ag_dst.data_ptr(), count=2048 * w,
                     dt=dtypes.FLOAT32, mem_type=dtypes.MEM_CUDA,
                     flags=c.FLAG_PERSISTENT, timeout=TIMEOUT)
    for rnd in range(2):
        pair(1, 2, 50 + rnd)
        # small allreduce (fused path)
        x = torch.full((1024,), float(r + 1 + rnd), device="cuda")
        y = torch.zeros(1024, device="cuda")
        torch.cuda.synchronize()
        j.ok([c.coll_init(team, "allreduce", src=x.data_ptr(),
                          dst=y.data_ptr(), count=1024, dt=dtypes.FLOAT32,
                          mem_type=dtypes.MEM_CUDA, timeout=TIMEOUT)])
        torch.cuda.synchronize()
        assert bool((y.cpu() == float(sum(q + 1 + rnd
                                          for q in range(w)))).all())
        # full-team bcast (staged_linear)
        src = payload(60 + rnd, 300_001)
        b = src.cuda() if r == 0 else \
            torch.zeros(300_001, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        j.n_bcast += 1
        j.ok([c.coll_init(team, "bcast", src=b.data_ptr(), dst=0,
                          count=300_001, dt=dtypes.UINT8, root=0,
                          mem_type=dtypes.MEM_CUDA, timeout=TIMEOUT)])
        expect(b, src, "interleave bcast")
        # persistent allgather (gated path)
        ag_src.fill_(float(10 * rnd + r))
        torch.cuda.synchronize()
        j.ok([ag])
        torch.cuda.synchronize()
        exp = torch.cat([torch.full((2048,), float(10 * rnd + q))
                         for q in range(w)])
        assert torch.equal(ag_dst.cpu(), exp), "interleave allgather"
        pair(2, 1, 70 + rnd)
        pair(3, 0, 80 + rnd)


def mismatch(j):
    """Tag mismatch (sender 7, receiver 9) and length mismatch on 0 -> 1:
    both ends fail well inside the timeout, the descriptor is consumed
    and the next transfer on the pair succeeds."""
    r = j.rank
    if r not in (0, 1):
        return
    n = 4096
    src = payload(90, n)
    buf = src.cuda() if r == 0 else \
        torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t0 = time.time()
    st = j.run([j.send(buf, 1, tag=7) if r == 0 else j.recv(buf, 0, tag=9)])
    assert st[0] < 0, ("tag mismatch", r, st)
    st = j.run([j.send(buf, 1, tag=3) if r == 0
                else j.recv(buf[:n // 2], 0, tag=3)])
    assert st[0] < 0, ("length mismatch", r, st)
    assert time.time() - t0 < TIMEOUT / 3, "mismatch was not prompt"
    j.ok([j.send(buf, 1, tag=4) if r == 0 else j.recv(buf, 0, tag=4)])
    expect(buf, src, "after mismatch")


def run_four():
    j = P2p()
    assert j.world == 4
    for case in (single_pair, both_directions, ring, active_sets,
                 persistent, interleave, mismatch):
        case(j)
        torch.cuda.synchronize()
        dist.barrier()
        if j.rank == 0:
            print(f"P2P4_CASE {case.__name__} ok", flush=True)
    j.finish("P2P4_OK")


# ------------------------------------------------------------- two ranks
def pipeline_case(j):
    """4 microbatches forward and backward, 64 KiB of bf16 each, then
    broadcast_stage_weights."""
    r = j.rank
    pp = PipelineStage(j.comm, timeout=TIMEOUT)
    n = 32 * 1024

    def bf16(seed):
        return payload(seed, 2 * n).view(torch.int16).cuda() \
            .view(torch.bfloat16)

    for mb in range(4):
        acts = bf16(200 + mb) if r == 0 else \
            torch.zeros(n, dtype=torch.bfloat16, device="cuda")
        pp.recv_forward(acts)
        pp.send_forward(acts)
        expect(acts, payload(200 + mb, 2 * n), f"forward {mb}")
        grads = bf16(300 + mb) if r == 1 else \
            torch.zeros(n, dtype=torch.bfloat16, device="cuda")
        pp.recv_backward(grads)
        pp.send_backward(grads)
        expect(grads, payload(300 + mb, 2 * n), f"backward {mb}")
    w = bf16(400) if r == 0 else \
        torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    torch.cuda.synchronize()
    pp.broadcast_stage_weights([w], root=0)
    expect(w, payload(400, 2 * n), "stage weights")
    return pp


def run_two(off):
    j = P2p()
    assert j.world == 2
    pp = pipeline_case(j)
    if off:
        assert pp.edge._device is False, "expected the host fallback"
        buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
        try:
            j.send(buf, 1) if j.rank == 0 else j.recv(buf, 0)
        except RuntimeError as e:
            assert "not supported" in str(e).lower(), e
        else:
            raise AssertionError("device active-set bcast was accepted "
                                 "with UCC_TL_CDNA4_P2P=0")
        j.n_p2p = 0
    else:
        assert pp.edge._device is True
        j.n_p2p = 8  # 4 forward + 4 backward transfers per rank
    j.finish("P2P2_OK")


# ----------------------------------------------------------- measurements
def run_bench():
    """PipelineEdge.send/recv round trips between 2 ranks. Uses nothing but
    the PipelineEdge API, so the same file measures a checkout where the
    edge still stages through the host."""
    torch.cuda.set_device(0)
    rank = int(os.environ["RANK"])
    dist.init_process_group("gloo", rank=rank,
                            world_size=int(os.environ["WORLD_SIZE"]))
    edge = PipelineEdge(Communicator())
    rows = []
    for nbytes in (8, 64 * 1024, MiB, 16 * MiB, 64 * MiB):
        t = torch.ones(nbytes // 2, dtype=torch.bfloat16, device="cuda")
        torch.cuda.synchronize()

        def trip():
            if rank == 0:
                edge.send(t, 1)
                edge.recv(t, 1)
            else:
                edge.recv(t, 0)
                edge.send(t, 0)

        for _ in range(20):
            trip()
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        for _ in range(100):
            trip()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 100
        rows.append(dict(bytes=nbytes, round_trip_us=dt * 1e6,
                         gbps_one_way=2 * nbytes / dt / 1e9))
    dist.barrier()
    if rank == 0:
        print("P2P_BENCH " + json.dumps(rows), flush=True)
    dist.destroy_process_group()


def run_sweep():
    """In-process pull-kernel time against the forced block count."""
    torch.cuda.set_device(0)
    c = core()
    rows = []
    for nbytes in (MiB, 64 * MiB):
        src = torch.ones(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        # two passes over the list: the second shows the spread
        for blocks in (1, 4, 16, 64, 128, 256, 0) * 2:
            for _ in range(5):
                used = c.ec_p2p_pull(dst.data_ptr(), src.data_ptr(), nbytes,
                                     blocks)
            iters = 10 if blocks == 1 and nbytes > MiB else 50
            t0 = time.perf_counter()
            for _ in range(iters):
                c.ec_p2p_pull(dst.data_ptr(), src.data_ptr(), nbytes,
                              blocks)
            dt = (time.perf_counter() - t0) / iters
            rows.append(dict(bytes=nbytes, blocks=blocks, used=used,
                             us=dt * 1e6, gbps=nbytes / dt / 1e9))
    print("P2P_SWEEP " + json.dumps(rows), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "four":
        run_four()
    elif mode in ("two", "two_off"):
        run_two(mode == "two_off")
    elif mode == "--bench":
        run_bench()
    elif mode == "--sweep":
        run_sweep()
    else:
        raise SystemExit(f"unknown mode {mode}")
