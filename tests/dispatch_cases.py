"""The dtype x op table of the device reductions and an exact host model of
it, shared by tests/test_ec_dispatch_gpu.py and tests/dispatch_worker.py.

Two ranks draw from {-2..2} (signed, float) or {0, 1, 2} (unsigned), so
every SUM, PROD, MAX, MIN and AVG result (halves, magnitude <= 4) and every
logical/bitwise result is exactly representable in every type down to
e5m2, and no integer overflows: the comparison needs no tolerance.
`expected()` asserts that by round-tripping its result through the dtype.
"""

import numpy as np
import torch

from ucc_amd import dtypes as D

INTS = {
    D.INT8: np.int8, D.UINT8: np.uint8, D.INT16: np.int16,
    D.UINT16: np.uint16, D.INT32: np.int32, D.UINT32: np.uint32,
    D.INT64: np.int64, D.UINT64: np.uint64,
}
NP_FLOATS = {D.FLOAT16: np.float16, D.FLOAT32: np.float32,
             D.FLOAT64: np.float64}
FP8 = {D.FLOAT8_E4M3: torch.float8_e4m3fn, D.FLOAT8_E5M2: torch.float8_e5m2}
COMPLEX = {D.FLOAT32_COMPLEX: np.complex64, D.FLOAT64_COMPLEX: np.complex128}
FLOATS = list(NP_FLOATS) + [D.BFLOAT16] + list(FP8)

NAMES = {v: k for k, v in vars(D).items()
         if isinstance(v, int) and not k.startswith(("OP_", "MEM_"))}
OP_NAMES = {v: k[3:] for k, v in vars(D).items() if k.startswith("OP_")}

ARITH = [D.OP_SUM, D.OP_PROD, D.OP_MAX, D.OP_MIN]
LOGIC = [D.OP_LAND, D.OP_LOR, D.OP_LXOR, D.OP_BAND, D.OP_BOR, D.OP_BXOR]
OPS = ARITH + LOGIC + [D.OP_AVG]
ALL_DTS = list(INTS) + FLOATS + list(COMPLEX)


def supported(dt, op):
    if dt in COMPLEX:
        return op in (D.OP_SUM, D.OP_AVG)
    if dt in FLOATS:
        return op in ARITH + [D.OP_AVG]
    return op in ARITH + LOGIC


CELLS = [(dt, op) for dt in ALL_DTS for op in OPS if supported(dt, op)]
UNSUPPORTED = [(dt, op) for dt in ALL_DTS for op in OPS
               if not supported(dt, op)]


def cell_id(cell):
    return f"{NAMES[cell[0]]}-{OP_NAMES[cell[1]]}"


def count_for(dt):
    """three 16-byte packs and a three-element scalar tail"""
    return 3 * (16 // D.DT_SIZE[dt]) + 3


def encode(dt, vals):
    """model values (int64 / float64 / complex128) -> raw bytes of dt"""
    if dt in INTS:
        return vals.astype(INTS[dt]).tobytes()
    if dt in NP_FLOATS:
        return vals.astype(NP_FLOATS[dt]).tobytes()
    if dt in COMPLEX:
        return vals.astype(COMPLEX[dt]).tobytes()
    if dt == D.BFLOAT16:
        u = vals.astype(np.float32).view(np.uint32) >> 16
        return u.astype(np.uint16).tobytes()
    t = torch.from_numpy(vals.astype(np.float32)).to(FP8[dt])
    return t.view(torch.uint8).numpy().tobytes()


def decode(dt, raw):
    """raw bytes of dt -> model values"""
    if dt in INTS:
        return np.frombuffer(raw, dtype=INTS[dt]).astype(np.int64)
    if dt in NP_FLOATS:
        return np.frombuffer(raw, dtype=NP_FLOATS[dt]).astype(np.float64)
    if dt in COMPLEX:
        return np.frombuffer(raw, dtype=COMPLEX[dt]).astype(np.complex128)
    if dt == D.BFLOAT16:
        u = np.frombuffer(raw, dtype=np.uint16).astype(np.uint32) << 16
        return u.view(np.float32).astype(np.float64)
    t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).view(FP8[dt])
    return t.float().numpy().astype(np.float64)


def inputs(dt, op, nranks=2):
    """[nranks, count] model values, seeded per cell"""
    rng = np.random.default_rng(1000 * dt + op)
    n = count_for(dt)
    unsigned = dt in INTS and np.dtype(INTS[dt]).kind == "u"
    lo = 0 if unsigned else -2

    def draw():
        return rng.integers(lo, 3, size=(nranks, n))

    if dt in COMPLEX:
        return draw() + 1j * draw()
    return draw().astype(np.int64 if dt in INTS else np.float64)


def expected(dt, op, x):
    a, b = x[0], x[1]
    if op == D.OP_SUM:
        r = a + b
    elif op == D.OP_AVG:
        r = (a + b) / 2
    elif op == D.OP_PROD:
        r = a * b
    elif op == D.OP_MAX:
        r = np.maximum(a, b)
    elif op == D.OP_MIN:
        r = np.minimum(a, b)
    elif op == D.OP_LAND:
        r = ((a != 0) & (b != 0)).astype(np.int64)
    elif op == D.OP_LOR:
        r = ((a != 0) | (b != 0)).astype(np.int64)
    elif op == D.OP_LXOR:
        r = ((a != 0) ^ (b != 0)).astype(np.int64)
    elif op == D.OP_BAND:
        r = a & b
    elif op == D.OP_BOR:
        r = a | b
    elif op == D.OP_BXOR:
        r = a ^ b
    else:
        raise ValueError(op)
    for v in (a, b, r):
        assert np.array_equal(decode(dt, encode(dt, v)), v), \
            f"{cell_id((dt, op))}: value set does not round-trip"
    return r


def to_device(dt, vals):
    raw = bytearray(encode(dt, vals))
    return torch.frombuffer(raw, dtype=torch.uint8).cuda()


def mismatch(dt, op, x, dst):
    """None if the device bytes in dst decode to exactly expected(),
    else a description of the difference"""
    got = decode(dt, dst.cpu().numpy().tobytes())
    exp = expected(dt, op, x)
    if got.shape == exp.shape and np.array_equal(got, exp):
        return None
    return f"{cell_id((dt, op))}: got {got.tolist()} expected {exp.tolist()}"
