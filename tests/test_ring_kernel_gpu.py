"""The ring-step kernel (src/ec/kernels/ec_ring.hip) in one process,
through the ec_ring_step binding: the five step forms of the multi-ring
schedule, for the 8/16-bit floats, f32 and int32, bit for bit.

Inputs are m * 2^-7 with integer |m| <= 256 (e4m3: m / 8, |m| <= 16), so
any f32 sum of up to 8 of them is exact in any order: the expected result
is float32 arithmetic on the CPU plus ONE conversion to the type (for e4m3
the model of tests/numerics_cases.py; AVG multiplies by float32(1 / n) in
float32 first). A travelling partial (`in` with in_acc, `out` with out_acc)
is raw float32. int32 accumulates in int32 and wraps.

Every output buffer sits between two 64-byte guard bands that must come
back unchanged, and every pointer is also shifted by one element of the
type stored behind it, one pointer at a time, which takes the piece off the
16-byte pack path onto the element-wise one."""

import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0xC3
# 0 and 1, one short of a bf16 pack, the pack, one over, and two 4-deep
# rounds of a 256-thread workgroup's 8-element packs plus a tail
COUNTS = (0, 1, 7, 8, 9, 2 * 256 * 8 * 4 + 5)


def _mods():
    from ucc_amd import core, dtypes
    import numerics_cases
    return core(), dtypes, numerics_cases


class Kind:
    """one dtype x op: value generation, the one conversion, the op"""

    def __init__(self, name, dt, op, nsum, alpha=1.0):
        self.name, self.dt, self.op = name, dt, op
        self.nsum = nsum      # values already folded into a partial
        self.alpha = alpha

    def setup(self, D, NC):
        self.D, self.NC = D, NC
        self.is_int = self.dt == D.INT32
        self.tsize = D.DT_SIZE[self.dt]
        self.asize = 4
        self.acc_np = np.int32 if self.is_int else np.float32

    def gen(self, rng, count, terms=1):
        """`terms` inputs folded in the accumulator type"""
        acc = None
        for _ in range(terms):
            if self.is_int:
                if self.op == self.D.OP_SUM:   # wraps around
                    v = rng.integers(2 ** 30, 2 ** 31 - 1, count,
                                     dtype=np.int64)
                    v = np.where(rng.integers(0, 2, count) == 1, v, -v)
                else:
                    v = rng.integers(-2 ** 31, 2 ** 31 - 1, count,
                                     dtype=np.int64)
                v = v.astype(np.int32)
            elif self.dt == self.D.FLOAT8_E4M3:
                v = (rng.integers(-16, 17, count) / 8.0).astype(np.float32)
            else:
                v = (rng.integers(-256, 257, count) / 128.0).astype(
                    np.float32)
            acc = v if acc is None else self.fold(acc, v)
        return acc

    def fold(self, a, b):
        if self.op == self.D.OP_MAX:
            return np.maximum(a, b)
        if self.is_int:
            return (a.astype(np.int64) + b.astype(np.int64)).astype(np.int32)
        return (a + b).astype(np.float32)

    def enc(self, acc, alpha=1.0):
        """accumulator values -> bytes of T: alpha, then ONE conversion"""
        D = self.D
        if self.is_int:
            return np.asarray(acc, dtype=np.int32).tobytes()
        acc = np.asarray(acc, dtype=np.float32)
        if alpha != 1.0:
            acc = (acc * np.float32(alpha)).astype(np.float32)
        if self.dt == D.FLOAT32:
            return acc.tobytes()
        if self.dt == D.FLOAT16:
            return acc.astype(np.float16).tobytes()
        if self.dt == D.BFLOAT16:
            t = torch.from_numpy(acc.copy()).to(torch.bfloat16)
            return t.view(torch.int16).numpy().tobytes()
        return self.NC._store(self.dt, acc)

    def raw(self, acc):
        return np.asarray(acc, dtype=self.acc_np).tobytes()


def _kinds(D):
    return [
        Kind("bf16_sum", D.BFLOAT16, D.OP_SUM, 6),
        Kind("fp16_sum", D.FLOAT16, D.OP_SUM, 6),
        Kind("f32_sum", D.FLOAT32, D.OP_SUM, 6),
        Kind("e4m3_sum", D.FLOAT8_E4M3, D.OP_SUM, 6),
        Kind("int32_max", D.INT32, D.OP_MAX, 6),
        Kind("int32_sum_wrap", D.INT32, D.OP_SUM, 6),
        Kind("bf16_avg_n3", D.BFLOAT16, D.OP_AVG, 2, alpha=1.0 / 3.0),
    ]


KIND_NAMES = ["bf16_sum", "fp16_sum", "f32_sum", "e4m3_sum", "int32_max",
              "int32_sum_wrap", "bf16_avg_n3"]

# form -> (in: None / "t" / "acc", local, out: None / "t" / "acc", dst,
#          final)
FORMS = {
    "copy_in": (None, True, "t", False, False),
    "middle_first": ("t", True, "acc", False, False),
    "middle": ("acc", True, "acc", False, False),
    "last_rs": ("acc", True, None, True, True),
    "last_rs_out": ("acc", True, "t", True, True),
    "last_rs_n2": ("t", True, None, True, True),
    "ag_out": ("t", False, "t", True, False),
    "ag_last": ("t", False, None, True, False),
}


class Buf:
    """bytes on the device between two guard bands, the payload shifted by
    `shift` bytes off 16-byte alignment"""

    def __init__(self, nbytes, shift, data=None):
        self.lo = GUARD + shift
        self.n = nbytes
        h = torch.full((GUARD + 16 + nbytes + GUARD,), SENTINEL,
                       dtype=torch.uint8)
        if data is not None:
            h[self.lo:self.lo + nbytes] = torch.frombuffer(
                bytearray(data), dtype=torch.uint8) if nbytes else h[0:0]
        self.d = h.cuda()
        assert self.d.data_ptr() % 16 == 0
        self.ptr = self.d.data_ptr() + self.lo

    def check(self, expect, what):
        got = self.d.cpu().numpy()
        body = got[self.lo:self.lo + self.n].tobytes()
        assert body == expect, what
        assert (got[:self.lo] == SENTINEL).all(), (what, "guard below")
        assert (got[self.lo + self.n:] == SENTINEL).all(), \
            (what, "guard above")


def _piece(kind, rng, form, count, shifts):
    """one piece: device buffers, the binding's tuple and the checks.
    shifts: set of pointer names moved by one element"""
    f_in, f_local, f_out, f_dst, final = FORMS[form]
    alpha = kind.alpha if final else 1.0
    tsz, asz = kind.tsize, kind.asize
    bufs, checks = {}, []
    acc = None
    if f_in:
        terms = kind.nsum if f_in == "acc" else 1
        v = kind.gen(rng, count, terms)
        data = kind.raw(v) if f_in == "acc" else kind.enc(v)
        esz = asz if f_in == "acc" else tsz
        bufs["in"] = Buf(count * esz, esz if "in" in shifts else 0, data)
        acc = v
    if f_local:
        v = kind.gen(rng, count)
        bufs["local"] = Buf(count * tsz, tsz if "local" in shifts else 0,
                            kind.enc(v))
        acc = v if acc is None else kind.fold(acc, v)
    t_bits = kind.enc(acc, alpha)
    if f_out:
        esz = asz if f_out == "acc" else tsz
        bufs["out"] = Buf(count * esz, esz if "out" in shifts else 0)
        checks.append((bufs["out"],
                       kind.raw(acc) if f_out == "acc" else t_bits, "out"))
    if f_dst:
        bufs["dst"] = Buf(count * tsz, tsz if "dst" in shifts else 0)
        checks.append((bufs["dst"], t_bits, "dst"))
    tup = tuple(bufs[k].ptr if k in bufs else 0
                for k in ("in", "local", "out", "dst")) + (count,)
    return tup, checks, bufs


def _run(c, kind, form, pieces, what, blocks=0):
    f_in, _, f_out, _, final = FORMS[form]
    tups = [p[0] for p in pieces]
    before = c.ec_ring_step_launches()
    torch.cuda.synchronize()
    st = c.ec_ring_step(tups, kind.dt, kind.op,
                        kind.alpha if final else 1.0,
                        1 if f_in == "acc" else 0,
                        1 if f_out == "acc" else 0, blocks)
    assert st == c.OK, what
    assert c.ec_ring_step_launches() == before + 1, what
    for k, p in enumerate(pieces):
        for buf, expect, name in p[1]:
            buf.check(expect, (what, "piece", k, name))


def _pointers(form):
    f_in, f_local, f_out, f_dst, _ = FORMS[form]
    return [n for n, used in (("in", f_in), ("local", f_local),
                              ("out", f_out), ("dst", f_dst)) if used]


@pytest.mark.parametrize("kname", KIND_NAMES)
def test_ring_step_forms_one_ring(kname):
    """every form x count, all pointers aligned and each pointer shifted
    alone, one piece per launch"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c, D, NC = _mods()
    kind = {k.name: k for k in _kinds(D)}[kname]
    kind.setup(D, NC)
    rng = np.random.default_rng(KIND_NAMES.index(kname) + 7)
    for form in FORMS:
        for count in COUNTS:
            for shifts in [set()] + [{p} for p in _pointers(form)]:
                if count == 0 and shifts:
                    continue
                what = (kname, form, count, sorted(shifts))
                _run(c, kind, form,
                     [_piece(kind, rng, form, count, shifts)], what)


@pytest.mark.parametrize("kname", KIND_NAMES)
def test_ring_step_forms_four_rings(kname):
    """four unequal pieces in one launch, one of them empty, one on the
    element-wise path; also a forced grid smaller than the pieces"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c, D, NC = _mods()
    kind = {k.name: k for k in _kinds(D)}[kname]
    kind.setup(D, NC)
    rng = np.random.default_rng(KIND_NAMES.index(kname) + 101)
    counts = (COUNTS[-1], 9, 0, 3 * 256 * 8 + 7)
    for form in FORMS:
        ptrs = _pointers(form)
        for blocks in (0, 3):
            pieces = [
                _piece(kind, rng, form, counts[0], set()),
                _piece(kind, rng, form, counts[1], set()),
                _piece(kind, rng, form, counts[2], set()),
                _piece(kind, rng, form, counts[3], {ptrs[-1]}),
            ]
            _run(c, kind, form, pieces, (kname, form, "4 rings", blocks),
                 blocks)


def test_ring_step_refuses_what_reduce_refuses():
    """a dtype x op outside the table is refused, not computed"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c, D, _ = _mods()
    a = torch.zeros(64, dtype=torch.float32, device="cuda")
    b = torch.zeros(64, dtype=torch.float32, device="cuda")
    o = torch.zeros(64, dtype=torch.float32, device="cuda")
    before = c.ec_ring_step_launches()
    st = c.ec_ring_step([(a.data_ptr(), b.data_ptr(), 0, o.data_ptr(), 64)],
                        D.FLOAT32, D.OP_BAND, 1.0, 0, 0)
    assert st != c.OK
    assert c.ec_ring_step_launches() == before
