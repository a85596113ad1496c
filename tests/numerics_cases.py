"""Edge-value cases for the reductions and an exact model of the documented
numerics (docs/USER_GUIDE.md, "Reduction numerics"), shared by
tests/test_reduce_numerics.py (host path), tests/test_reduce_numerics_gpu.py
and tests/numerics_worker.py (device paths). Pure numpy / torch on the CPU.

For n ranks, cases(n) yields messages: per (family, dtype, op) the raw input
bit patterns of every rank and the expected output bit patterns. The
expectation is worked out from first principles:

 * the exact value of the reduction in float64 (Python ints for integers);
 * for AVG one multiplication by np.float32(1.0 / n) in float32, or by
   1.0 / n in float64 for FLOAT64 / FLOAT64_COMPLEX;
 * for the fp8 types the clamp of a finite value to +-max-finite;
 * ONE round-to-nearest-even conversion to the type (torch / numpy casts,
   which are only ever fed the clamped value).

The comparison is bit-exact. That is legitimate because every float column
is checked here to be independent of the accumulation order: the running
float32 (float64 for the 64-bit types) result is identical in rank order and
in reversed rank order and equals the float64 (exact rational) result. A
violated assertion in this file is a bug in a case, not in the library.
NaN results compare as "is a NaN encoding of the type".

MAX / MIN with a NaN operand or a +0 / -0 tie are unspecified and must not
occur in a case; the builder asserts that too.
"""

from fractions import Fraction

import numpy as np
import torch

from ucc_amd import dtypes as D

from dispatch_cases import (COMPLEX, FLOATS, FP8, INTS, NAMES, NP_FLOATS,
                            OP_NAMES, decode, encode)

# narrow float formats: explicit mantissa bits, min normal exponent, max finite
NARROW = {
    D.BFLOAT16: (7, -126, (2.0 - 2.0 ** -7) * 2.0 ** 127),
    D.FLOAT16: (10, -14, 65504.0),
    D.FLOAT8_E4M3: (3, -6, 448.0),
    D.FLOAT8_E5M2: (2, -14, 57344.0),
}
F64_TYPES = (D.FLOAT64, D.FLOAT64_COMPLEX)
UINT_OF = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
NAN, INF = float("nan"), float("inf")

# classes of stored values that every store site must see (narrow floats;
# the wide types only have nan and negzero)
EDGE_CLASSES = ("tie_down", "tie_up", "off", "subnormal", "ovf+", "ovf-",
                "nan", "negzero")


def comp_dt(dt):
    """the real type a complex type is made of (dt itself otherwise)"""
    return {D.FLOAT32_COMPLEX: D.FLOAT32,
            D.FLOAT64_COMPLEX: D.FLOAT64}.get(dt, dt)


def vec_of(dt):
    return 16 // D.DT_SIZE[dt]


def bits_of(dt, raw):
    """raw bytes -> unsigned words, one per real component"""
    return np.frombuffer(raw, dtype=UINT_OF[D.DT_SIZE[comp_dt(dt)]])


def _same(a, b):
    """same float value including the sign of zero; NaN equals NaN"""
    a, b = np.float64(a), np.float64(b)
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    return bool(a == b and np.signbit(a) == np.signbit(b))


def _step(dt, v, k):
    """the representable value k steps of magnitude away from v > 0"""
    w = bits_of(dt, encode(dt, np.array([v], dtype=np.float64)))
    w = np.array([int(w[0]) + k], dtype=w.dtype)
    return float(decode(dt, w.tobytes())[0])


# ------------------------------------------------------------ the model
def _store(dt, acc):
    """accumulator values (float32, or float64 for FLOAT64) -> raw bytes:
    fp8 clamp, then one round-to-nearest-even conversion"""
    if dt == D.FLOAT64:
        return np.asarray(acc, dtype=np.float64).tobytes()
    acc = np.asarray(acc, dtype=np.float32)
    if dt == D.FLOAT32:
        return acc.tobytes()
    if dt == D.FLOAT16:
        with np.errstate(over="ignore"):
            return acc.astype(np.float16).tobytes()
    if dt == D.BFLOAT16:
        t = torch.from_numpy(acc.copy()).to(torch.bfloat16)
        return t.view(torch.int16).numpy().tobytes()
    big = np.float32(NARROW[dt][2])
    acc = np.where(np.isfinite(acc), np.clip(acc, -big, big), acc)
    t = torch.from_numpy(acc.astype(np.float32)).to(FP8[dt])
    return t.view(torch.uint8).numpy().tobytes()


def _fold(vals, op, ftype):
    with np.errstate(all="ignore"):
        acc = ftype(vals[0])
        for v in vals[1:]:
            v = ftype(v)
            acc = acc + v if op != D.OP_PROD else acc * v
        return acc


def _accumulate(dt, op, col, what):
    """the accumulator value of one real column (before AVG's scale), with
    the order-independence and exactness assertions"""
    n = len(col)
    if op in (D.OP_MAX, D.OP_MIN):
        assert not any(np.isnan(v) for v in col), f"{what}: NaN in MAX/MIN"
        assert sum(1 for v in col if v == 0) <= 1, f"{what}: +-0 tie"
        return max(col) if op == D.OP_MAX else min(col)
    ftype = np.float64 if dt in F64_TYPES else np.float32
    fwd = _fold(col, op, ftype)
    rev = _fold(col[::-1], op, ftype)
    assert _same(fwd, rev), f"{what}: order dependent {col}"
    if ftype is np.float32:
        assert _same(fwd, _fold(col, op, np.float64)), \
            f"{what}: float32 accumulation inexact {col}"
    elif all(np.isfinite(v) for v in col):
        exact = Fraction(col[0])
        for v in col[1:]:
            exact = exact + Fraction(v) if op != D.OP_PROD \
                else exact * Fraction(v)
        assert Fraction(float(fwd)) == exact, \
            f"{what}: float64 accumulation inexact {col}"
    assert n >= 1
    return fwd


def _result(dt, op, col, what):
    """accumulator value at the store of one real column"""
    rdt = comp_dt(dt)
    acc = _accumulate(rdt, op, col, what)
    if op == D.OP_AVG:
        with np.errstate(all="ignore"):
            if rdt == D.FLOAT64:
                acc = np.float64(acc) * np.float64(1.0 / len(col))
            else:
                acc = np.float32(acc) * np.float32(1.0 / len(col))
    return acc


def _classes(dt, acc):
    """store-edge classes of one accumulator value"""
    acc = float(acc)
    if np.isnan(acc):
        return {"nan"}
    out = set()
    rdt = comp_dt(dt)
    stored = float(decode(rdt, _store(rdt, [acc]))[0])
    if stored == 0 and np.signbit(stored):
        out.add("negzero")
    if dt not in NARROW or np.isinf(acc):
        return out
    m, emin, big = NARROW[dt]
    if abs(acc) > big:
        out.add("ovf+" if acc > 0 else "ovf-")
        return out
    if acc != 0 and abs(acc) < 2.0 ** emin:
        out.add("subnormal")
    if stored != acc:
        a, r = abs(acc), abs(stored)
        other = _step(dt, r, -1 if r > a else 1) if r > 0 \
            else 2.0 ** (emin - m)
        if Fraction(a) - Fraction(min(r, other)) == \
                Fraction(max(r, other)) - Fraction(a):
            out.add("tie_down" if r < a else "tie_up")
        else:
            out.add("off")
    return out


# --------------------------------------------------------------- layout
def _layouts(ncols, classes, vec):
    """element -> column index arrays. Every column sits in a full 16-byte
    pack; every class present sits in the scalar tail of some layout;
    count % vec != 0 wherever the type has a tail at all."""
    packs = -(-ncols // vec) * vec
    head = [i % ncols for i in range(packs)]
    if vec == 1:
        return [np.array(head)]
    cover = []
    for k in EDGE_CLASSES:
        if any(k in c for c in classes) and \
                not any(k in classes[i] for i in cover):
            cover.append(next(i for i, c in enumerate(classes) if k in c))
    if not cover:
        cover = [i % ncols for i in range(min(vec - 1, 3))]
    outs = []
    for b in range(0, len(cover), vec - 1):
        tail = cover[b:b + vec - 1]
        idx = np.array(head + tail)
        assert len(idx) % vec != 0
        outs.append(idx)
    tails = set()
    for idx in outs:
        for i in idx[packs:]:
            tails |= classes[i]
    present = set().union(*classes) if classes else set()
    assert present <= tails | set(), "a store-edge class misses the tail"
    assert all(set(range(ncols)) <= set(idx[:packs].tolist())
               for idx in outs)
    return outs


class Case:
    """one message: x[r] raw src bytes of rank r, exp raw expected bytes"""

    def __init__(self, family, dt, op, n, tag, x, exp, classes):
        self.family, self.dt, self.op, self.n = family, dt, op, n
        self.x, self.exp, self.classes = x, exp, classes
        self.count = len(exp) // D.DT_SIZE[dt]
        self.nbytes = len(exp)
        self.id = f"{family}-{NAMES[dt]}-{OP_NAMES[op]}-n{n}{tag}"

    def mismatch(self, got):
        """None if the raw result bytes equal the expectation (any NaN
        encoding where a NaN is expected), else a description"""
        got = bytes(got)
        if len(got) != len(self.exp):
            return f"{self.id}: {len(got)} bytes, expected {len(self.exp)}"
        g, e = bits_of(self.dt, got), bits_of(self.dt, self.exp)
        ok = g == e
        if self.dt not in INTS:
            rdt = comp_dt(self.dt)
            ok |= np.isnan(decode(rdt, self.exp)) & \
                np.isnan(decode(rdt, got))
        if ok.all():
            return None
        bad = np.flatnonzero(~ok)
        return (f"{self.id}: component(s) {bad.tolist()} got "
                f"{[hex(int(v)) for v in g[bad]]} expected "
                f"{[hex(int(v)) for v in e[bad]]}")


def _float_cases(family, dt, op, n, cols):
    """cols: list of n-tuples of float (complex for the complex types)"""
    what = f"{family}-{NAMES[dt]}-{OP_NAMES[op]}-n{n}"
    assert cols and all(len(c) == n for c in cols), what
    rdt = comp_dt(dt)
    accs, classes = [], []
    for c in cols:
        if dt in COMPLEX:
            parts = [_result(dt, op, tuple(complex(v).real for v in c), what),
                     _result(dt, op, tuple(complex(v).imag for v in c), what)]
        else:
            parts = [_result(dt, op, tuple(float(v) for v in c), what)]
        accs.append(parts)
        classes.append(set().union(*(_classes(rdt, p) for p in parts)))
    vals = np.ascontiguousarray(
        np.array(cols, dtype=np.complex128 if dt in COMPLEX
                 else np.float64).T)            # [n, ncols]
    with np.errstate(all="ignore"):
        for r in range(n):                      # inputs are representable
            back = decode(dt, encode(dt, vals[r]))
            for a, b in zip(back.view(np.float64), vals[r].view(np.float64)):
                assert _same(a, b), f"{what}: input {b} not representable"
    out = []
    lays = _layouts(len(cols), classes, vec_of(dt))
    for k, idx in enumerate(lays):
        with np.errstate(all="ignore"):
            x = [encode(dt, vals[r][idx]) for r in range(n)]
        flat = [p for i in idx for p in accs[i]]
        exp = _store(rdt, np.array(flat, dtype=np.float64 if rdt == D.FLOAT64
                                   else np.float32))
        tag = f"-L{k}" if len(lays) > 1 else ""
        out.append(Case(family, dt, op, n, tag, x, exp,
                        set().union(*classes)))
    return out


def _pad(head, n, ident):
    assert len(head) <= n
    return tuple(head) + (ident,) * (n - len(head))


def _ident(op):
    return 1.0 if op == D.OP_PROD else 0.0


# -------------------------------------------------------------- families
def _ties(dt, op, n):
    """v with even / odd last mantissa bit (and all ones: the carry into the
    next binade) plus exactly half an ulp, and half an ulp +- a sliver. For
    AVG the ranks hold n*v in binary pieces and n*ulp/2: sum * f32(1/n) is
    then v + ulp/2 again (checked by the class assertion in cases()).

    At n = 7 that only holds below 4/3 of a power of two: 7 * f32(1/7) is
    1 + 0.75 * 2^-24, so for a larger mantissa the float32 product is one
    float32 ulp above v + ulp/2 and no longer a tie. e5m2 has a single
    midpoint below 4/3 (1.125, between the even 1.0 and 1.25), so its
    7-rank AVG ties go down only; no choice of inputs gives it a tie that
    goes up. cases() asserts tie_up at n = 7 for the other three types."""
    m = NARROW[dt][0]
    u = 2.0 ** -m
    cols = []
    for v in (1.0, 1.0 + u, 2.0 - u, 1.5):
        for k in (0, 1, -1):
            for sgn in (1.0, -1.0):
                if op == D.OP_SUM:
                    d = _step(dt, u / 2, k) if k else u / 2
                    head = [v, d]
                else:
                    d = _step(dt, n * u / 2, k) if k else n * u / 2
                    head = [v * 2.0 ** b for b in range(8) if n >> b & 1]
                    head.append(d)
                cols.append(_pad([sgn * h for h in head], n, 0.0))
    return cols


def _subnormal(dt, op, n):
    m, emin, _ = NARROW[dt]
    s, mn = 2.0 ** (emin - m), 2.0 ** emin
    if op == D.OP_SUM:
        heads = [(s, 2 * s), (-s, -2 * s), (mn - s, s), (mn, -s),
                 (s, -2 * s), (-mn, s), (2 * s, s)]
    elif op == D.OP_AVG:
        # sum = j * s: j = 1 underflows to 0 (-1 to -0), 2 lands in
        # (s/2, s) at n = 3, the others inside the subnormal range
        heads = [(float(j // 2) * s, float(j - j // 2) * s)
                 for j in (1, 2, 4, 5, 7, 8, n, 2 * n, -1, -2, -4, -5, -7)]
    else:
        # s * 0.5 is the tie at half the minimum subnormal (-> 0, even);
        # s * next(0.5) and s * 0.625 are just above it (-> s)
        heads = [(s, 0.5), (s, _step(dt, 0.5, 1)), (s, 0.625), (s, 1.5),
                 (s, 2.5), (-s, 0.5), (-s, 0.625), (mn, 0.5), (mn, -0.75),
                 (s, _step(dt, 0.5, -1)), (-s, 1.5)]
    return [_pad(h, n, _ident(op)) for h in heads]


def _overflow(dt, op, n):
    m, _, big = NARROW[dt]
    u = 2.0 ** (int(np.floor(np.log2(big))) - m)
    heads = []
    for sgn in (1.0, -1.0):
        if op == D.OP_SUM:
            # just below / at / just above the rounding threshold big + u/2,
            # and a full ulp above
            for d in (_step(dt, u / 2, -1), u / 2, _step(dt, u / 2, 1), u):
                if dt == D.BFLOAT16 and d == u:
                    continue  # max(bf16) + u is not finite in float32
                heads.append((sgn * big, sgn * d))
            if dt in FP8:
                heads.append((sgn * big, sgn * big, sgn * big))
        else:
            heads.append((sgn * big, 2.0))
            heads.append((big / 2, sgn * 4.0))
    return [_pad(h, n, _ident(op)) for h in heads]


def _specials(dt, op, n):
    has_inf = comp_dt(dt) != D.FLOAT8_E4M3
    if op in (D.OP_SUM, D.OP_AVG):
        heads = [(NAN, 1.0, 2.0), (-0.0, -0.0, -0.0), (1.5, -1.5, 0.0),
                 (1.5, 2.0, 0.5), (-3.0, 1.0, 0.5)]
        if has_inf:
            heads += [(INF, 1.0, 2.0), (-INF, 1.0, -2.0), (INF, -INF, 1.0)]
        if op == D.OP_AVG:  # -0 needs every rank to hold -0
            heads[1] = (-0.0,) * n
    elif op == D.OP_PROD:
        heads = [(NAN, 1.0, 2.0), (-0.0, 2.0, 1.0), (-1.0, 0.0, 2.0),
                 (-0.0, -1.0, 1.0), (1.5, 2.0, -1.0)]
        if has_inf:
            heads += [(INF, 2.0, 1.0), (INF, -2.0, 1.0), (INF, 0.0, 1.0)]
    else:
        heads = [(3.0, -1.0, 2.0), (-3.0, -1.5, -2.0), (0.0, -1.0, 2.0),
                 (-0.0, 1.0, 2.0)]
        if has_inf:
            heads += [(INF, 1.0, -2.0), (-INF, 1.0, 2.0), (-INF, INF, 0.0)]
        else:
            heads += [(448.0, -448.0, 1.0)]
        return [_pad(h, n, h[1]) for h in heads]
    cols = [_pad(h, n, _ident(op)) for h in heads]
    if dt in COMPLEX:   # imaginary parts: the next column's values
        cols = [tuple(complex(a, b) for a, b in
                      zip(c, cols[(i + 1) % len(cols)]))
                for i, c in enumerate(cols)]
    return cols


def _avg_scale(dt, op, n):
    """integer-valued inputs whose sum is no multiple of n: the stored bits
    depend on the precision of 1/n"""
    rng = np.random.default_rng(7000 + 10 * dt + n)
    lim = {D.BFLOAT16: 64, D.FLOAT32: 10 ** 6, D.FLOAT32_COMPLEX: 10 ** 6}
    lim = lim.get(dt, 10 ** 12)

    def draw():
        v = rng.integers(-lim, lim + 1, size=(11, n))
        for row in v:
            if row.sum() % n == 0:
                row[0] += 1 if row[0] < lim else -1
        assert (v.sum(axis=1) % n != 0).all()
        return v.astype(np.float64)

    if dt in COMPLEX:
        return [tuple(c) for c in draw() + 1j * draw()]
    return [tuple(c) for c in draw()]


def _int_cases(dt, op, n):
    npdt = np.dtype(INTS[dt])
    bits = 8 * npdt.itemsize
    mask = (1 << bits) - 1
    signed = npdt.kind == "i"
    hi = 1 << (bits - 1)
    tmax, tmin = (hi - 1, -hi) if signed else (mask, 0)

    def val(w):
        w &= mask
        return w - (1 << bits) if signed and w & hi else w

    if op in (D.OP_MAX, D.OP_MIN):
        cols = [(tmin, tmax, 0), (-1, 0, hi), (tmax, -1, hi), (hi, hi - 1, 0),
                (hi - 1, hi + 1, 1), (-1, hi, hi + 1), (tmin, 0, -1),
                (1, hi - 1, hi)]
    elif op == D.OP_SUM:
        cols = [(tmax, 1, 0), (tmin, -1, 0), (tmax, tmax, tmax),
                (hi, hi, 0), (-1, -1, -1), (hi - 1, hi - 1, 2), (5, -7, 1)]
    elif op == D.OP_PROD:
        cols = [(tmax, 2, 1), (hi, 2, 1), (-1, tmin, 1), (3, tmax, 5),
                (hi - 1, hi - 1, 3), (-1, -1, -1), (1 << (bits // 2), 1 <<
                                                    (bits // 2), 1)]
    elif op in (D.OP_BAND, D.OP_BOR, D.OP_BXOR):
        rng = np.random.default_rng(9000 + 10 * dt + op)
        cols = [tuple(int.from_bytes(rng.bytes(npdt.itemsize), "little")
                      for _ in range(n)) for _ in range(11)]
    else:
        # non-zero operands whose low byte is zero (where the type has
        # more than one byte)
        a, b, c = ((0x80, 0x10, 0x40) if bits == 8 else
                   (0x100, hi, 1 << (bits - 8)))
        cols = [(a, b, c), (a, 0, c), (a, 0, 0), (0, 0, 0), (0, b, 0),
                (hi, hi, 0), (0, c, b)]
    assert n == 3 and all(len(c) == n for c in cols)
    exp = []
    for c in cols:
        v = [val(w) for w in c]
        if op == D.OP_MAX:
            r = max(v)
        elif op == D.OP_MIN:
            r = min(v)
        elif op == D.OP_SUM:
            r = sum(v)
        elif op == D.OP_PROD:
            r = 1
            for w in v:
                r *= w
        elif op == D.OP_BAND:
            r = mask
            for w in v:
                r &= w
        elif op == D.OP_BOR:
            r = 0
            for w in v:
                r |= w
        elif op == D.OP_BXOR:
            r = 0
            for w in v:
                r ^= w
        elif op == D.OP_LAND:
            r = int(all(w != 0 for w in v))
        elif op == D.OP_LOR:
            r = int(any(w != 0 for w in v))
        else:
            r = sum(1 for w in v if w != 0) & 1
        exp.append(r & mask)
    udt = UINT_OF[npdt.itemsize]
    idx = _layouts(len(cols), [set()] * len(cols), vec_of(dt))[0]
    x = [np.array([cols[i][r] & mask for i in idx], dtype=udt).tobytes()
         for r in range(n)]
    e = np.array([exp[i] for i in idx], dtype=udt).tobytes()
    return [Case("intext", dt, op, n, "", x, e, set())]


# ---------------------------------------------------------------- tables
NARROW_DTS = list(NARROW)
ALL_FLOATS = FLOATS + list(COMPLEX)
INT_OPS = [D.OP_SUM, D.OP_PROD, D.OP_MAX, D.OP_MIN, D.OP_LAND, D.OP_LOR,
           D.OP_LXOR, D.OP_BAND, D.OP_BOR, D.OP_BXOR]

# classes a family must produce for every narrow type at n = 3
REQUIRED = {
    ("ties", D.OP_SUM): {"tie_down", "tie_up", "off"},
    ("ties", D.OP_AVG): {"tie_down", "tie_up", "off"},
    ("subnormal", D.OP_SUM): {"subnormal"},
    ("subnormal", D.OP_AVG): {"subnormal", "off", "negzero"},
    ("subnormal", D.OP_PROD): {"subnormal", "tie_down", "tie_up", "off",
                               "negzero"},
    ("overflow", D.OP_SUM): {"ovf+", "ovf-"},
    ("specials", D.OP_SUM): {"nan", "negzero"},
    ("specials", D.OP_AVG): {"nan", "negzero"},
    ("specials", D.OP_PROD): {"nan", "negzero"},
}


def _family_table(n):
    """(family, builder, dtypes, ops) rows that run at n ranks"""
    rows = [
        ("ties", _ties, NARROW_DTS, [D.OP_SUM, D.OP_AVG]),
        ("subnormal", _subnormal, NARROW_DTS,
         [D.OP_SUM, D.OP_AVG, D.OP_PROD]),
        ("overflow", _overflow, NARROW_DTS, [D.OP_SUM, D.OP_PROD]),
        ("specials", _specials, ALL_FLOATS,
         [D.OP_SUM, D.OP_PROD, D.OP_AVG, D.OP_MAX, D.OP_MIN]),
        ("avgscale", _avg_scale,
         [D.FLOAT32, D.FLOAT64, D.FLOAT32_COMPLEX, D.FLOAT64_COMPLEX,
          D.BFLOAT16], [D.OP_AVG]),
    ]
    if n != 3:   # the AVG cases also run at n = 7
        rows = [(f, b, dts, [D.OP_AVG]) for f, b, dts, ops in rows
                if D.OP_AVG in ops]
    return rows


_CACHE = {}


def cases(n):
    """every message that runs at n ranks (built once per n)"""
    if n in _CACHE:
        return _CACHE[n]
    out = []
    for family, build, dts, ops in _family_table(n):
        for dt in dts:
            for op in ops:
                if dt in COMPLEX and op not in (D.OP_SUM, D.OP_AVG):
                    continue
                if family == "overflow" and op == D.OP_PROD and \
                        dt == D.BFLOAT16:
                    continue  # 2 * max(bf16) is not finite in float32
                got = _float_cases(family, dt, op, n, build(dt, op, n))
                need = REQUIRED.get((family, op), set())
                if dt in NARROW and n == 3:
                    have = set().union(*(c.classes for c in got))
                    assert need <= have, \
                        f"{got[0].id}: classes {need - have} missing"
                elif family == "ties":
                    have = set().union(*(c.classes for c in got))
                    need = {"tie_down", "off"} | \
                        ({"tie_up"} if NARROW[dt][0] >= 3 else set())
                    assert need <= have, \
                        f"{got[0].id}: classes {need - have} missing"
                elif family == "specials" and need:
                    have = set().union(*(c.classes for c in got))
                    assert {"nan", "negzero"} <= have, got[0].id
                out += got
    if n == 3:
        for dt in INTS:
            for op in INT_OPS:
                out += _int_cases(dt, op, n)
    assert len({c.id for c in out}) == len(out)
    assert all(16 < c.nbytes <= 512 for c in out)
    _CACHE[n] = out
    return out


def is_scalar_family(c):
    """the cases the unaligned (scalar kernel) path runs: narrow floats and
    the integer extremes"""
    return c.dt in NARROW or c.dt in INTS


MIN_BYTES = 17  # every message is at least one 16-byte pack plus a tail
