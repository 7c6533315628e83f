"""Shared inputs of the point / proof decoder tests (csrc/zl_decode.h, zl_decode_dev.hip): per curve and group one set of compressed records that
reaches every status of the host decoder and every select of the lane-uniform one, the host decoder's answer for each of them (zl_point_from_bytes, the
yardstick), and the Fq2 values of the square-root hook.  Built once per process and never changed."""
import ctypes as C
import functools
import random

import numpy as np

import oracle_lib as ol
from oracle_lib import po
from openzl_amd import backend as zb

CURVES = [po.BLS12_381, po.BN254]
OK, EINVAL, ENOTCURVE = 0, -1, -6


def nb(curve) -> int:
    """bytes per Fq element on the wire"""
    return 48 if curve.cid == 1 else 32


def g1_limbs(curve, P):
    nq = ol.nlq(curve)
    return np.array(ol.ints_to_limbs([P[0], P[1]], nq)).reshape(-1) if P is not None else np.zeros(2 * nq, dtype=np.uint64)


def g2_limbs(curve, P):
    nq = ol.nlq(curve)
    if P is None:
        return np.zeros(4 * nq, dtype=np.uint64)
    return np.array(ol.ints_to_limbs([P[0][0], P[0][1], P[1][0], P[1][1]], nq)).reshape(-1)


def _neg2(curve, P):
    p = curve.fq.p
    return (P[0], ((p - P[1][0]) % p, (p - P[1][1]) % p))


def _fq(curve, x: int, flags: int = 0) -> bytes:
    """x as one wire element (it must fit below the flag bits), flags in the top two bits of the last byte"""
    out = bytearray(x.to_bytes(nb(curve), "little"))
    assert out[-1] & 0xC0 == 0
    out[-1] |= flags
    return bytes(out)


def in_subgroup(curve, group: int, P) -> bool:
    """r P = infinity by the oracle's arithmetic.  Its g1_mul / g2_mul reduce the scalar mod r first (r P would be 0 P), so: (r - 1) P + P"""
    mul, add = (po.g1_mul, po.g1_add) if group == 1 else (po.g2_mul, po.g2_add)
    return add(curve, mul(curve, curve.fr.p - 1, P), P) is None


def _rhs1(curve, x):
    return (x * x * x + curve.b) % curve.fq.p


def _rhs2(curve, x):
    p = curve.fq.p
    return po.f2_add(p, po.f2_mul(p, po.f2_mul(p, x, x), x), curve.b2)


@functools.lru_cache(maxsize=None)
def _records(cid: int, group: int):
    curve = next(c for c in CURVES if c.cid == cid)
    p, r, n = curve.fq.p, curve.fr.p, nb(curve)
    rng = random.Random(0xDEC0DE + 10 * cid + group)
    recs = []  # (label, bytes, status the construction implies or None)
    if group == 1:
        G, mul, add, neg = po.g1_generator(curve), po.g1_mul, po.g1_add, po.g1_neg
        limbs, compress = g1_limbs, po.g1_compress
    else:
        G, mul, add, neg = po.g2_generator(curve), po.g2_mul, po.g2_add, _neg2
        limbs, compress = g2_limbs, po.g2_compress
    # valid subgroup points, both sign flags, compressed by the library
    valid = []
    for k in [1, 2, r - 1] + [rng.randrange(3, r - 1) for _ in range(3)]:
        P = mul(curve, k, G)
        for Q in (P, neg(curve, P)):
            data = zb.point_to_bytes(cid, group, limbs(curve, Q))
            assert data == compress(curve, Q)
            recs.append(("valid", data, OK))
            valid.append(Q)
    inf = zb.point_to_bytes(cid, group, limbs(curve, None), inf=1)
    recs.append(("infinity", inf, OK))
    g = bytearray(compress(curve, G))
    recs.append(("inf_flag_x_nonzero", bytes(g[:-1]) + bytes([(g[-1] & 0x3F) | 0x40]), EINVAL))
    recs.append(("both_flags", bytes(g[:-1]) + bytes([g[-1] | 0xC0]), EINVAL))
    recs.append(("both_flags_x_zero", bytes(group * n - 1) + bytes([0xC0]), EINVAL))
    lead = b"" if group == 1 else _fq(curve, 1)  # G2: a fine c0 in front of the element under test (c1 carries the flags)
    for name, x in (("x_eq_q", p), ("x_eq_q_plus_1", p + 1), ("x_all_ones", (1 << (8 * n - 2)) - 1)):
        recs.append((name, lead + _fq(curve, x), EINVAL))
        recs.append((name + "_big", lead + _fq(curve, x, 0x80), EINVAL))
    recs.append(("x_eq_q_inf_flag", lead + _fq(curve, p, 0x40), EINVAL))
    recs.append(("x_eq_q_minus_1", lead + _fq(curve, p - 1), None))  # whatever the host decoder says
    if group == 2:
        c1 = _fq(curve, G[0][1])
        recs.append(("c0_flag_big", _fq(curve, G[0][0], 0x80) + c1, EINVAL))
        recs.append(("c0_flag_inf", _fq(curve, G[0][0], 0x40) + c1, EINVAL))
        recs.append(("c0_eq_q", _fq(curve, p) + c1, EINVAL))
        recs.append(("c0_all_ones", _fq(curve, (1 << (8 * n - 2)) - 1) + c1, EINVAL))
        recs.append(("c0_eq_q_minus_1", _fq(curve, p - 1) + c1, None))
    # x without a y, and curve points outside the subgroup: the smallest x = 1, 2, ... (G2: x = (i, 1)) of each kind, both sign flags
    no_y, outside, i = [], [], 0
    while len(no_y) < 2 or (len(outside) < 2 and not (cid == 2 and group == 1)) or i < 4:
        i += 1
        if group == 1:
            y = po.fq_sqrt(p, _rhs1(curve, i))
            x, xb = i, _fq(curve, i)
        else:
            x = (i, 1)
            y = po.f2_sqrt(p, _rhs2(curve, x))
            xb = _fq(curve, i) + _fq(curve, 1)
        if y is None:
            if len(no_y) < 2:
                no_y.append(x)
                recs.append(("no_y", xb, ENOTCURVE))
                recs.append(("no_y_big", xb[:-1] + bytes([xb[-1] | 0x80]), ENOTCURVE))
            continue
        P = (x, y)
        in_group = in_subgroup(curve, group, P)
        if cid == 2 and group == 1:
            assert in_group, "BN254 G1 has cofactor 1: every curve point is in the subgroup"
        if in_group:
            recs.append(("valid_small_x", compress(curve, P), OK))
            valid.append(P)
        elif len(outside) < 2:
            outside.append(P)
            for Q in (P, neg(curve, P)):
                recs.append(("outside_subgroup", compress(curve, Q), ENOTCURVE))
    if outside:  # subgroup + non-subgroup: still outside, with coordinates that are not small
        for P in outside:
            S = add(curve, valid[6], P)
            assert not in_subgroup(curve, group, S)
            recs.append(("outside_subgroup_large", compress(curve, S), ENOTCURVE))
    return tuple(recs)


def records(curve, group: int):
    """((label, bytes, status implied by the construction or None), ...) of one curve and group, about 40"""
    return _records(curve.cid, group)


def valid_records(curve, group: int):
    return [rec for label, rec, st in records(curve, group) if st == OK and label != "infinity"]


def first(curve, group: int, label: str) -> bytes:
    return next(rec for lab, rec, _ in records(curve, group) if lab == label)


def host_decode(curve, group: int, recs):
    """the existing host decoder (zl_point_from_bytes) on every record: (xy (n, words), inf (n,), status (n,)) -- the expected value of every decoder test"""
    L = zb.load_library()
    words = 2 * group * ol.nlq(curve)
    xy = np.zeros((len(recs), words), dtype=np.uint64)
    inf = np.zeros(len(recs), dtype=np.uint8)
    st = np.zeros(len(recs), dtype=np.int32)
    for i, rec in enumerate(recs):
        buf = (C.c_uint8 * len(rec)).from_buffer_copy(rec)
        one = C.c_uint8(0)
        st[i] = L.zl_point_from_bytes(curve.cid, group, buf, zb._p64(xy[i]), C.byref(one))
        inf[i] = one.value
    return xy, inf, st


@functools.lru_cache(maxsize=None)
def _expected(cid: int, group: int):
    curve = next(c for c in CURVES if c.cid == cid)
    recs = [rec for _, rec, _ in records(curve, group)]
    xy, inf, st = host_decode(curve, group, recs)
    for a in (xy, inf, st):
        a.setflags(write=False)
    return xy, inf, st


def expected(curve, group: int):
    """host_decode of records(curve, group), computed once (read-only arrays)"""
    return _expected(curve.cid, group)


def host_proof(curve, data: bytes):
    """zl_groth16_proof_from_bytes on one record: (status, the struct as the call leaves it)"""
    pc = zb.G16ProofC()
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    st = zb.load_library().zl_groth16_proof_from_bytes(curve.cid, buf, len(data), C.byref(pc))
    return st, pc


def proof_fields(pc):
    return bytes(pc.a), bytes(pc.b), bytes(pc.c), pc.a_inf, pc.b_inf, pc.c_inf


@functools.lru_cache(maxsize=None)
def _sqrt_inputs(cid: int):
    curve = next(c for c in CURVES if c.cid == cid)
    p = curve.fq.p
    rng = random.Random(0x5A17 + cid)
    s, t = rng.randrange(2, p), rng.randrange(2, p)
    nonres = next(v for v in range(2, 100) if po.fq_sqrt(p, v) is None)
    vals = [(0, 0), (1, 0), (s * s % p, 0), ((p - s * s) % p, 0), (nonres, 0), ((p - nonres) % p, 0), (0, t), (0, p - t), (0, 1)]
    squares, others = [], []
    while len(squares) < 6 or len(others) < 6:
        a = (rng.randrange(p), rng.randrange(1, p))
        if len(squares) < 6:
            squares.append(po.f2_mul(p, a, a))
        if po.f2_sqrt(p, a) is None and len(others) < 6:
            others.append(a)
    return tuple(vals + squares + others)


def sqrt_inputs(curve):
    """Fq2 values (c0, c1) of the square-root hook: zero, real squares and non-squares of Fq (both square in Fq2), purely imaginary values, random
    squares and random non-squares"""
    return _sqrt_inputs(curve.cid)


def fq2_words(curve, vals) -> np.ndarray:
    nq = ol.nlq(curve)
    return np.array(ol.ints_to_limbs([c for v in vals for c in v], nq), dtype=np.uint64).reshape(len(vals), 2 * nq)


def check_sqrt(curve, vals, roots, ok):
    p, nq = curve.fq.p, ol.nlq(curve)
    for v, row, good in zip(vals, roots, ok):
        exp = po.f2_sqrt(p, v)
        assert bool(good) == (exp is not None), v
        r = tuple(ol.limbs_to_ints(np.asarray(row).reshape(2, nq)))
        if good:
            assert r[0] < p and r[1] < p and po.f2_mul(p, r, r) == v, v
        else:
            assert r == (0, 0), v
