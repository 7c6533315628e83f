"""Operand sets and the Python-integer reference of the carry-chain field tests (zl_test_fp_op: Fp<P> of openzl_amd/csrc/zl_field.h and Fp2<P> of
zl_curve.h on raw limbs).  The hook converts and reduces nothing, so every value below is the integer of the N raw words: mul(a, b) is a b R^-1 mod p with
R = 2^(32 N), to_mont(a) is a R mod p, and so on.  Nothing here calls the library; the host and the device tests share one set of cases per field."""
import functools
import random

import numpy as np

from oracle_lib import po

# field ids of zl_test_fp_op
BLS_FR, BLS_FQ, BN_FR, BN_FQ = 0, 1, 2, 3
# ops
MUL, SQR, ADD, SUB, DBL, NEG, TO_MONT, FROM_MONT, INV, IS_ZERO, EQ, REDUCE_ONCE, FROM_U64 = range(13)
MUL2, SQR2, INV2, ADD2, SUB2, NEG2, TO_MONT2, FROM_MONT2 = range(20, 28)


class Field:
    def __init__(self, fid, name, p, curve):
        self.fid, self.name, self.p, self.curve = fid, name, p, curve
        self.bits = p.bit_length()
        self.N = 2 * ((self.bits + 63) // 64)  # 32-bit words of R = 2^(64 ceil(bits / 64))
        self.R = 1 << (32 * self.N)
        self.Rinv = pow(self.R, -1, p)
        self.INV = (-pow(p, -1, 1 << 32)) % (1 << 32)  # -p^-1 mod 2^32: the Montgomery quotient word is m = t0 INV
        self.has_fp2 = fid in (BLS_FQ, BN_FQ)

    def __repr__(self):
        return self.name


FIELDS = [Field(BLS_FR, "bls12_381_fr", po.BLS12_381.fr.p, po.BLS12_381), Field(BLS_FQ, "bls12_381_fq", po.BLS12_381.fq.p, po.BLS12_381),
          Field(BN_FR, "bn254_fr", po.BN254.fr.p, po.BN254), Field(BN_FQ, "bn254_fq", po.BN254.fq.p, po.BN254)]


def words(vals, n_words: int) -> np.ndarray:
    """integers -> (len, n_words) uint32, little-endian words"""
    buf = b"".join(int(v).to_bytes(4 * n_words, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u4").reshape(len(vals), n_words).astype(np.uint32)


def records(F: Field, quads) -> np.ndarray:
    """[(a, b, c, d)] integers -> (n, 4, N) uint32 records of the hook; shorter tuples are padded with 0"""
    flat = [v for q in quads for v in (tuple(q) + (0, 0, 0, 0))[:4]]
    return words(flat, F.N).reshape(len(quads), 4, F.N)


def ints(rows: np.ndarray):
    """(n, W) uint32 -> integers"""
    rows = np.ascontiguousarray(rows, dtype="<u4")
    return [int.from_bytes(r.tobytes(), "little") for r in rows]


# ---- the reference: Python integers only ----------------------------------------------------------------------------------------------------------------
def ref(F: Field, op: int, a: int, b: int = 0, c: int = 0, d: int = 0):
    """the result of one op on raw words: an integer (Fp ops, predicates 0 / 1) or a pair (c0, c1) (Fp2 ops, Fq[u] / (u^2 + 1))"""
    p, R, Ri = F.p, F.R, F.Rinv
    if op == MUL: return a * b * Ri % p
    if op == SQR: return a * a * Ri % p
    if op == ADD: return (a + b) % p
    if op == SUB: return (a - b) % p
    if op == DBL: return 2 * a % p
    if op == NEG: return -a % p
    if op == TO_MONT: return a * R % p
    if op == FROM_MONT: return a * Ri % p
    if op == INV: return pow(a * Ri % p, -1, p) * R % p if a % p else 0
    if op == IS_ZERO: return int(a == 0)
    if op == EQ: return int(a == b)
    if op == REDUCE_ONCE: return a - p if a >= p else a
    if op == FROM_U64: return (a & ((1 << 64) - 1)) * R % p
    if op == MUL2: return ((a * c - b * d) * Ri % p, (a * d + b * c) * Ri % p)
    if op == SQR2: return ((a * a - b * b) * Ri % p, 2 * a * b * Ri % p)
    if op == INV2:
        A, B = a * Ri % p, b * Ri % p
        n = pow((A * A + B * B) % p, -1, p)
        return (A * n * R % p, -B * n * R % p)
    if op == ADD2: return ((a + c) % p, (b + d) % p)
    if op == SUB2: return ((a - c) % p, (b - d) % p)
    if op == NEG2: return (-a % p, -b % p)
    if op == TO_MONT2: return (a * R % p, b * R % p)
    if op == FROM_MONT2: return (a * Ri % p, b * Ri % p)
    raise ValueError(op)


def expected(F: Field, op: int, quads) -> np.ndarray:
    """(n, N) or (n, 2 N) uint32: what the hook must write for the records `quads`"""
    out = [ref(F, op, *((tuple(q) + (0, 0, 0, 0))[:4])) for q in quads]
    if op >= MUL2:
        return words([v for pair in out for v in pair], F.N).reshape(len(quads), 2 * F.N)
    return words(out, F.N)


def cios_drops_carry(F: Field, a: int, b: int, limb_bits: int) -> bool:
    """whether a CIOS Montgomery product with multiplicand a (the operand every row multiplies) and rows taken from b, kept in exactly N words, loses a
    carry: the running value T_i = (a (b mod w^i) + M_i p) / w^i stays below a + p, which fits the N words for a < p and need not for a >= p.  limb_bits = 32
    (the portable loop) or 64 (the host's).  Used only to CHOOSE inputs at which an implementation that put an unreduced value first would be wrong."""
    w = 1 << limb_bits
    ninv = (-pow(F.p, -1, w)) % w
    t = 0
    for i in range(32 * F.N // limb_bits):
        t += a * ((b >> (limb_bits * i)) % w)
        t += (t * ninv % w) * F.p
        t >>= limb_bits
        if t >= F.R:
            return True
    return False


# ---- operand sets ---------------------------------------------------------------------------------------------------------------------------------------
def _rng(F: Field, tag: int):
    return random.Random(0xF1E1D000 + 16 * F.fid + tag)


@functools.lru_cache(maxsize=None)
def edge_set(F: Field):
    """E: canonical values at which carries, borrows and the final subtraction take their rare turns"""
    p, N = F.p, F.N
    top = p >> (32 * (N - 1))
    rnd = _rng(F, 0)
    E = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, F.R % p, F.R * F.R % p, 1 << (F.bits - 1), (1 << (F.bits - 1)) - 1]
    for j in range(1, N):
        E += [v for v in (1 << (32 * j), (1 << (32 * j)) - 1) if v < p]
    E.append(((top - 1) << (32 * (N - 1))) | ((1 << (32 * (N - 1))) - 1))  # every limb below the top one all ones
    # pairs whose first Montgomery quotient word m0 = a0 b0 INV mod 2^32 is 0 (a0 b0 = 0 mod 2^32, neither word 0) and 0xFFFFFFFF (a0 b0 = p0 mod 2^32)
    hi = lambda: rnd.randrange(p >> 32) << 32
    a0 = rnd.randrange(1 << 32) | 1
    E += [hi() | 0x00010000, hi() | 0xABCD0000, hi() | a0, hi() | ((p % (1 << 32)) * pow(a0, -1, 1 << 32) % (1 << 32))]
    E = list(dict.fromkeys(E))
    assert all(0 <= v < p for v in E)
    m0 = {(x % (1 << 32)) * (y % (1 << 32)) * F.INV % (1 << 32) for x in E[-4:] for y in E[-4:]}
    assert 0 in m0 and 0xFFFFFFFF in m0
    return tuple(E)


@functools.lru_cache(maxsize=None)
def wide_set(F: Field):
    """X: N-word values at or above p"""
    p, R = F.p, F.R
    rnd = _rng(F, 1)
    X = [p, p + 1, 2 * p - 1, 2 * p, R - 1, R - 2, R - p, R - 1 - p] + [rnd.randrange(p, R) for _ in range(20)]
    assert all(p <= v < R for v in X)
    return tuple(X)


def _pairs(S, T=None):
    return [(a, b) for a in S for b in (S if T is None else T)]


@functools.lru_cache(maxsize=None)
def fp_cases(F: Field):
    """{name: (op, [(a, b, c, d)])} for the Fp ops; a name that ends in '@X' holds operands at or above p (the multiplier's contract: a < p, b any N words)"""
    p, N, R = F.p, F.N, F.R
    E, X = edge_set(F), wide_set(F)
    rnd = _rng(F, 2)
    rand_pairs = [(rnd.randrange(p), rnd.randrange(p)) for _ in range(2000)]
    cases = {"mul": (MUL, _pairs(E) + rand_pairs), "sqr": (SQR, [(a,) for a in E] + [(a,) for a, _ in rand_pairs]),
             "mul@X": (MUL, _pairs(E, X) + [(rnd.randrange(p), rnd.randrange(p, R)) for _ in range(200)])}
    # sums on p - 1, p, p + 1; differences -1, 0 and a borrow through j equal limbs; doubles on p - 1 and p + 1
    sums = [(a, t - a) for a in E for t in (p - 1, p, p + 1) if 0 <= t - a < p]
    diffs = [(a, a + 1) for a in E if a + 1 < p] + [(a, a) for a in E]
    diffs += [(1 << (32 * j), 1) for j in range(1, N) if (1 << (32 * j)) < p] + [(1, 1 << (32 * j)) for j in range(1, N) if (1 << (32 * j)) < p]
    for j in range(1, N):  # limbs 1 .. j - 1 equal in a and b (a random word each), limb 0 borrows: the borrow walks through them into limb j, from either side
        same = sum(rnd.randrange(1 << 32) << (32 * i) for i in range(1, j))
        hi_a, hi_b = sorted((rnd.randrange(1, (p >> (32 * j)) or 2), rnd.randrange(1, (p >> (32 * j)) or 2)), reverse=True)
        a, b = (hi_a << (32 * j)) | same, ((hi_b << (32 * j)) | same) + 1
        diffs += [(a, b), (b, a)]
    halves = [((p - 1) // 2, (p - 1) // 2), ((p + 1) // 2, (p + 1) // 2)]
    assert all(a < p and b < p for a, b in sums + diffs)
    cases["add"] = (ADD, _pairs(E) + sums + halves + rand_pairs[:200])
    cases["sub"] = (SUB, _pairs(E) + diffs + rand_pairs[:200])
    cases["dbl"] = (DBL, [(a,) for a in E] + [(a,) for a, _ in halves] + [(a,) for a, _ in rand_pairs[:200]])
    cases["neg"] = (NEG, [(a,) for a in E] + [(a,) for a, _ in rand_pairs[:200]])
    # reduce_once on [0, 2p): the ends, and values that share their top j limbs with p (the borrow decides in limb N - 1 - j)
    red = [0, p - 1, p, p + 1, 2 * p - 1]
    for j in range(1, N):
        keep = (p >> (32 * (N - j))) << (32 * (N - j))
        low = 1 << (32 * (N - j))
        red += [keep, keep | (low - 1), keep | rnd.randrange(low), keep | ((p % low) - 1) % low, keep | ((p % low) + 1) % low]
    red += [p + a for a in E] + list(E)
    red = [v for v in dict.fromkeys(red) if v < 2 * p and v < R]
    cases["reduce_once"] = (REDUCE_ONCE, [(a,) for a in red])
    inv_in = [0, 1, 2, p - 1] + [rnd.randrange(1, p) for _ in range(16)]
    cases["inv"] = (INV, [(a,) for a in inv_in])
    cases["is_zero"] = (IS_ZERO, [(a,) for a in E] + [(1 << (32 * j),) for j in range(N)])
    cases["eq"] = (EQ, _pairs(E[:12]) + [(a, a ^ (1 << (32 * j))) for a in E[:6] for j in range(N)])
    conv = list(E) + [a for a, _ in rand_pairs[:200]]
    cases["to_mont"] = (TO_MONT, [(a,) for a in conv])
    cases["from_mont"] = (FROM_MONT, [(a,) for a in conv])
    cases["from_u64"] = (FROM_U64, [(a,) for a in conv] + [((1 << 64) - 1,), (1 << 63,), (1 << 32,), ((1 << 32) - 1,)])
    cases["to_mont@X"] = (TO_MONT, [(a,) for a in X])
    cases["from_mont@X"] = (FROM_MONT, [(a,) for a in X])
    cases["from_u64@X"] = (FROM_U64, [(a,) for a in X])
    return cases


@functools.lru_cache(maxsize=None)
def fp2_cases(F: Field):
    """{name: (op, [(a, b, c, d)])}, x = (a, b), y = (c, d): components from a 12-element subset of E so that c0 + c1 and c0 - c1 inside mul and sqr land on
    p and on 0, the shapes (x, 0), (0, x), (x, x), (x, p - x), and 200 random pairs"""
    assert F.has_fp2
    p = F.p
    E, X = edge_set(F), wide_set(F)
    rnd = _rng(F, 3)
    S = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, F.R % p, F.R * F.R % p, (1 << (F.bits - 1)) - 1, E[-1], E[-2]]
    elems = _pairs(S)
    shaped = [e for x in E for e in ((x, 0), (0, x), (x, x), (x, (p - x) % p))]
    rand = [tuple(rnd.randrange(p) for _ in range(4)) for _ in range(200)]
    ys = [(1, 0), (0, 1), (p - 1, p - 1), ((p + 1) // 2, (p - 1) // 2), (F.R % p, 0), (rnd.randrange(p), rnd.randrange(p))]
    binary = [x + y for x in elems for y in ys] + [x + y for x in shaped for y in shaped[:24]] + rand
    unary = [x + (0, 0) for x in elems + shaped] + rand
    nonzero = [q for q in unary if q[0] or q[1]]
    cases = {"fp2_mul": (MUL2, binary), "fp2_sqr": (SQR2, unary), "fp2_inv": (INV2, nonzero[:150] + rand), "fp2_add": (ADD2, binary), "fp2_sub": (SUB2, binary),
             "fp2_neg": (NEG2, unary), "fp2_to_mont": (TO_MONT2, unary), "fp2_from_mont": (FROM_MONT2, unary),
             "fp2_to_mont@X": (TO_MONT2, [(a, b) for a in X[:10] for b in (0, p - 1) + X[:4]] + [(a, b) for b in X[:10] for a in (0, p - 1)])}
    return cases


def all_cases(F: Field):
    c = dict(fp_cases(F))
    if F.has_fp2:
        c.update(fp2_cases(F))
    return c


def is_wide(name: str) -> bool:
    return name.endswith("@X")


# ---- points whose coordinates are written x + k q -------------------------------------------------------------------------------------------------------
def k_max(F: Field, x: int) -> int:
    """the largest k for which x + k p still fits N words"""
    return (F.R - 1 - x) // F.p


def fq_of(curve) -> Field:
    return FIELDS[BLS_FQ] if curve is po.BLS12_381 else FIELDS[BN_FQ]


def rewrite_coord(curve, xy: np.ndarray, coord: int, k: int) -> np.ndarray:
    """a copy of the canonical u64 words `xy` (coordinates of nlq words each) with coordinate `coord` written as its value + k q"""
    F = fq_of(curve)
    nq = F.N // 2
    out = np.array(xy, dtype=np.uint64, copy=True).reshape(-1)
    v = int.from_bytes(out[coord * nq:(coord + 1) * nq].astype("<u8").tobytes(), "little") + k * F.p
    assert v < F.R
    out[coord * nq:(coord + 1) * nq] = np.frombuffer(v.to_bytes(8 * nq, "little"), dtype="<u8")
    return out.reshape(np.shape(xy))


def coord_int(curve, xy: np.ndarray, coord: int) -> int:
    nq = fq_of(curve).N // 2
    return int.from_bytes(np.asarray(xy, dtype="<u8").reshape(-1)[coord * nq:(coord + 1) * nq].tobytes(), "little")


def pick_lossy(curve, pts, coords):
    """the first (row, coordinate of `coords`) of `pts` whose value, written with the largest k that fits, is one at which a conversion that multiplies it
    FIRST into R^2 would lose a carry in the host's 64-bit loop (cios_drops_carry): (row index, coordinate, k).  About one value in twenty is."""
    F = fq_of(curve)
    r2 = F.R * F.R % F.p
    for i, row in enumerate(pts):
        for coord in coords:
            x = coord_int(curve, row, coord)
            k = k_max(F, x)
            if cios_drops_carry(F, x + k * F.p, r2, 64):
                return i, coord, k
    raise AssertionError("no candidate loses a carry: widen the candidate list")


@functools.lru_cache(maxsize=None)
def case_arrays(F: Field, name: str):
    """(op, records (n, 4, N), expected rows) of one case of all_cases(F): built once, shared by every form and by host and device"""
    op, quads = all_cases(F)[name]
    rec, exp = records(F, quads), expected(F, op, quads)
    rec.setflags(write=False)
    exp.setflags(write=False)
    return op, rec, exp


def wrong_rows(got: np.ndarray, exp: np.ndarray) -> int:
    return int((np.asarray(got) != np.asarray(exp)).any(axis=1).sum())
