"""The LANE FORMS of the lazily reduced Fq / Fq2 arithmetic at their contract bounds (openzl_amd/csrc/zl_fq2pair.h, zl_quad.h).

Since round 6 every G2 MSM and every small or mid-sized MSM computes on two layers of cross-lane arithmetic: Fp2H (an Fq2 element split over lanes i and
i ^ 8, partner operands by DPP row_ror:8 with bank masks, un-carried scan-only operands 32q - b1 / X < 32q / Y < 48q, predicates combined over the pair) and
add_full_quad / add_mixed_quad (one XYZZ addition over the four lanes of a quad; over Fp2H: eight lanes, an "octet").  tests/test_field28_bounds.py drives
the scalar forms with operands at the contract maxima; this file does the same for the lane forms through zl_test_fp2pair_op and zl_test_point_form_op,
which place items on lanes and in memory as the MSM kernels do.  The reference is Python big integers throughout:
  field level   the Fq2 product in Montgomery form, residue + "< 2q" + normalised limbs (the three checks of _check_field), every split of the component
                bounds up to 16q with the edges chosen independently per component; predicates on every raw-zero / == 0 mod q / non-zero combination;
                every batch holds its records twice, 19 items apart modulo 32 (a low and a high row of the wave), and ends in a partial wave;
  point level   the case matrix of _check_points (generic, P + P, P - P, infinity on either side or both; lifts to [7q, 8q), canonical, mixed) interleaved so
                that one wave holds all branches side by side, plus OFF-CURVE records that separate the halves of a pair: u1 and u2 agree in one component
                only (must stay generic), pp == 0 with r zero in one component only (must give infinity, not a doubling).  Expected values: a restatement of
                add-2008-s / madd-2008-s / the a = 0 doublings, compared projectively.
The model the GPU tests trust is itself verified without a GPU (test_*_host): the same generator and expectations run against the host path of the scalar
forms (the existing BLS12-381 hook and the BN254 host path of the new one), the restatement is compared with the group law of the oracle on every on-curve
record, and the Fq2 product model is composed from host zl_test_fp28_op / zl_test_fp28_bn_op calls.
Op 6 (to_affine) runs on the scalar and quad forms only: Fp2H has no inversion (no kernel leaves the XYZZ form on lane pairs; the hook returns ZL_EINVAL).
"""
import functools

import numpy as np
import pytest

from oracle_lib import po
from openzl_amd.backend import (FORM_OCTET, FORM_PAIR, FORM_QUAD, FORM_SCALAR, FORM_SCALAR_HOT, ZL_BLS12_381, ZL_BN254, ZL_G1, ZL_G2, hook_fp28_op,
                                hook_fp2pair_op, hook_point_form_op, hook_point_op)
from test_field28_bounds import BLS_FQ, BN_FQ, M28, edge_values, from_limbs, to_limbs

CURVES = {"bls12_381": (BLS_FQ, po.BLS12_381, ZL_BLS12_381), "bn254": (BN_FQ, po.BN254, ZL_BN254)}
CURVE_IDS = list(CURVES)


# ---- field level -------------------------------------------------------------------------------------------------------------------------
def _fq2_limbs(cfg, v):
    return np.concatenate([to_limbs(v[0], cfg.L), to_limbs(v[1], cfg.L)])


def _fq2_ints(cfg, o):
    return from_limbs(o[:cfg.L]), from_limbs(o[cfg.L:])


def _mont_mul2(cfg, a, b):
    """(a0 + a1 u)(b0 + b1 u) / R' mod q on raw (lazily reduced) integers"""
    return ((a[0] * b[0] - a[1] * b[1]) * cfg.RP_INV % cfg.Q, (a[0] * b[1] + a[1] * b[0]) * cfg.RP_INV % cfg.Q)


def _edges(cfg, bound, rng):
    """component values <= bound * q at the edges: k q - 1, k q, k q + 1, bound q - small, 0, 1 (edge_values) and, for the full contract, 16q itself"""
    return edge_values(bound, rng, 14, cfg.Q)


def _layout(records):
    """The batch a hook call runs: every record twice, the second copy 19 items later modulo 32 -- two rows of 16 lanes further on in its wave and on another
    lane of the row -- and a last wave that is partial.  Returns (rows, index of the first copy, index of the second copy)."""
    m = len(records)
    pad = (19 - m) % 32
    rows = list(records) + [records[(3 * i) % m] for i in range(pad)] + list(records)
    if len(rows) % 32 == 0:
        rows.append(records[0])
    assert (m + pad) % 32 == 19 and len(rows) % 32 != 0
    return rows, 0, m + pad


def _run_pair(be, cfg, cid, op, records):
    """records: tuples of up to four Fq2 operands (pairs of raw integers) -> per record the two results (both placements in the wave), as integer pairs + limbs"""
    rows, first, second = _layout(records)
    arr = np.zeros((len(rows), 4, 2 * cfg.L), dtype=np.uint32)
    for i, row in enumerate(rows):
        for j, v in enumerate(row):
            arr[i, j] = _fq2_limbs(cfg, v)
    out = hook_fp2pair_op(be, cid, op, arr)
    return [(out[first + i], out[second + i]) for i in range(len(records))]


def _field_product_records(cfg):
    """mul / sqr / muladd records: (op, operands, bounds).  Fixed seed; every component edge is chosen independently of the other component's."""
    Q = cfg.Q
    rng = np.random.Generator(np.random.PCG64(62))
    recs = []
    corner = [0, 1, Q, 16 * Q - 1, 16 * Q, 16 * Q - int(rng.integers(1, 1 << 62))]
    for ba, bb in [(1, 1), (2, 2), (8, 2), (2, 8), (10, 10), (16, 1), (1, 16), (16, 8), (8, 16), (16, 16)]:
        EA, EB = _edges(cfg, ba, rng), _edges(cfg, bb, rng)
        na, nb = len(EA), len(EB)
        for i in range(44):
            a = (EA[i % na], EA[(3 * i + 1) % na])
            b = (EB[(5 * i + 2) % nb], EB[(7 * i + 3) % nb])
            recs.append((0, (a, b), (ba, bb)))
    # the corners of the contract, all combinations: b1 = 0 and b1 = 16q (the un-carried 32q - b1), a0 = a1, one component 0 and the other 16q
    for a0 in corner:
        for a1 in corner:
            for b0 in (0, Q + 1, 16 * Q):
                for b1 in (0, 1, 16 * Q - 1, 16 * Q):
                    recs.append((0, ((a0, a1), (b0, b1)), (16, 16)))
    for ba in (1, 2, 8, 10, 16):
        EA = _edges(cfg, ba, rng)
        for a0 in EA:
            for a1 in EA[::2] + [a0]:
                recs.append((1, ((a0, a1),), (ba,)))
    for a0 in corner:
        for a1 in corner:
            recs.append((1, ((a0, a1),), (16,)))
    for bs in [(10, 10, 8, 2), (6, 10, 2, 8), (16, 16, 16, 16), (16, 1, 1, 16), (2, 16, 16, 2)]:
        E = [_edges(cfg, b, rng) for b in bs]
        for i in range(44):
            ops = tuple((E[k][(i * (2 * k + 3) + k) % len(E[k])], E[k][(i * (2 * k + 5) + 2 * k + 1) % len(E[k])]) for k in range(4))
            recs.append((2, ops, bs))
    for b1 in (0, 16 * Q):
        for d1 in (0, 16 * Q):
            for a in ((16 * Q, 16 * Q), (0, 16 * Q), (16 * Q, 0), (16 * Q - 1, 1)):
                recs.append((2, (a, (16 * Q, b1), a[::-1], (Q - 1, d1)), (16, 16, 16, 16)))
    return recs


def _product_expect(cfg, op, ops):
    if op == 0:
        return _mont_mul2(cfg, ops[0], ops[1])
    if op == 1:
        return _mont_mul2(cfg, ops[0], ops[0])
    x, y = _mont_mul2(cfg, ops[0], ops[1]), _mont_mul2(cfg, ops[2], ops[3])
    return ((x[0] + y[0]) % cfg.Q, (x[1] + y[1]) % cfg.Q)


def _predicate_records(cfg):
    """(c0, c1) over every kind of component: raw zero, == 0 mod q but not raw (q, 2q, 7q), non-zero (x, x + q) -- (0,0), (q,0), (0,q), (q,2q), (0,x), (x,0), (x,y)
    and all their raw / non-raw variants -- shuffled with a fixed seed so that neighbouring pairs of a wave hold different cases"""
    Q = cfg.Q
    rng = np.random.Generator(np.random.PCG64(63))
    x, y = int.from_bytes(rng.bytes(32), "little") % (Q - 1) + 1, int.from_bytes(rng.bytes(32), "little") % (Q - 1) + 1
    kinds0, kinds1 = [0, Q, 2 * Q, 7 * Q, x, x + Q, 1], [0, Q, 2 * Q, 7 * Q, y, y + 3 * Q, Q - 1]
    recs = [((c0, c1),) for c0 in kinds0 for c1 in kinds1]
    order = rng.permutation(len(recs))
    return [recs[i] for i in order]


def _check_normalised(cfg, o, strict_top):
    L = cfg.L
    for h in range(2):
        c = o[h * L:(h + 1) * L]
        assert (c[:L - 1] <= M28).all()
        if strict_top:
            assert c[L - 1] <= M28


def _check_pair_field(be, cfg, cid):
    Q, L = cfg.Q, cfg.L
    recs = _field_product_records(cfg)
    for op in (0, 1, 2):
        mine = [r for r in recs if r[0] == op]
        assert len(mine) > 100
        outs = _run_pair(be, cfg, cid, op, [r[1] for r in mine])
        for (_, ops, bounds), both in zip(mine, outs):
            exp = _product_expect(cfg, op, ops)
            for place, o in enumerate(both):
                v = _fq2_ints(cfg, o)
                info = ("fp2pair", cid, "op", op, "bounds", bounds, "operand multiples of q", [(c[0] // Q, c[1] // Q) for c in ops], "placement", place)
                assert v[0] < 2 * Q and v[1] < 2 * Q, info
                assert (o <= M28).all(), info
                assert (v[0] % Q, v[1] % Q) == exp, info
    rng = np.random.Generator(np.random.PCG64(64))

    def exact(op, records, fn, strict_top=False):
        for ops, both in zip(records, _run_pair(be, cfg, cid, op, records)):
            for o in both:
                assert _fq2_ints(cfg, o) == fn(*ops), ("fp2pair", cid, "op", op, [(c[0] // Q, c[1] // Q) for c in ops])
                _check_normalised(cfg, o, strict_top)

    def comp(fn):
        return lambda *ops: (fn(*[o[0] for o in ops]), fn(*[o[1] for o in ops]))

    A, Bv = edge_values(1000, rng, 24, Q), edge_values(1000, rng, 24, Q)
    exact(3, [((A[i], A[(i + 5) % 24]), (Bv[(i + 2) % 24], Bv[(7 * i) % 24])) for i in range(24)], comp(lambda a, b: a + b))
    exact(4, [((A[i], A[(i + 5) % 24]),) for i in range(24)], comp(lambda a: 2 * a))
    for J in range(1, 7):
        Bv = edge_values(1 << J, rng, 24, Q)
        A = edge_values(64, rng, len(Bv), Q)
        n = len(Bv)
        exact(4 + J, [((A[i], 0 if i % 3 == 0 else A[(i + 1) % n]), (Bv[(i + 3) % n], Bv[i])) for i in range(n)], comp(lambda a, b, J=J: a - b + (Q << J)))
        exact(16 + J, [((Bv[i], Bv[(5 * i + 1) % n]),) for i in range(n)], comp(lambda a, J=J: (Q << J) - a))
    E2 = edge_values(2, rng, 24, Q)
    E2 = [min(v, 2 * Q - 1) for v in E2]
    exact(15, [((E2[i], E2[(i + 1) % 24]), (E2[(3 * i) % 24], E2[(5 * i + 2) % 24]), (E2[(7 * i + 1) % 24], E2[(i + 9) % 24])) for i in range(24)]
          + [((0, 2 * Q - 1), (2 * Q - 1, 0), (2 * Q - 1, 0)), ((0, 0), (2 * Q - 1, 2 * Q - 1), (2 * Q - 1, 2 * Q - 1))], comp(lambda a, b, c: a - b - 2 * c + 6 * Q))
    W = edge_values(2000, rng, 40, Q) + [k * Q for k in (2, 3, 4, 5, 100, 1999, 2000)] + [k * Q + 1 for k in (3, 4, 1999)] + [k * Q - 1 for k in (1, 4, 2000)]
    wrec = [((W[i], W[(7 * i + 3) % len(W)]),) for i in range(len(W))]
    for (a,), both in zip(wrec, _run_pair(be, cfg, cid, 11, wrec)):
        for o in both:
            v = _fq2_ints(cfg, o)
            assert max(v) < 4 * Q and (v[0] % Q, v[1] % Q) == (a[0] % Q, a[1] % Q) and (o <= M28).all(), ("fp2pair", cid, "wred", a[0] // Q, a[1] // Q)
    exact(12, wrec, comp(lambda a: a % Q), strict_top=True)
    for both in _run_pair(be, cfg, cid, 16, [((5, 7),), ((0, 0),), ((Q, 1),)]):
        for o in both:
            v = _fq2_ints(cfg, o)
            assert v[0] < 2 * Q and v[0] % Q == cfg.RP % Q and not o[L:].any() and (o <= M28).all(), ("fp2pair", cid, "one")
    # predicates, combined over the pair: 0 / 1 in limb 0 of BOTH halves
    prec = _predicate_records(cfg)
    for op, fn in ((13, lambda a: a[0] % Q == 0 and a[1] % Q == 0), (14, lambda a: a == (0, 0))):
        exp = [int(fn(r[0])) for r in prec]
        assert 0 < sum(exp) < len(exp) and any(exp[i] != exp[i + 1] for i in range(len(exp) - 1))
        for (a,), e, both in zip(prec, exp, _run_pair(be, cfg, cid, op, prec)):
            for o in both:
                assert int(o[0]) == e and int(o[L]) == e and not o[1:L].any() and not o[L + 1:].any(), ("fp2pair", cid, "predicate", op, a[0] // Q, a[1] // Q, a[0] % Q == 0, a[1] % Q == 0)


# ---- point level -------------------------------------------------------------------------------------------------------------------------
class _Field:
    """Fq (deg 1: integers) or Fq2 (deg 2: pairs) of one curve: plain big-integer arithmetic + the raw-limb embedding (Montgomery, lifted by multiples of q)"""

    def __init__(self, cfg, deg):
        self.cfg, self.deg, self.Q, self.L, self.W = cfg, deg, cfg.Q, cfg.L, cfg.L * deg
        self.ZERO = 0 if deg == 1 else (0, 0)
        self.ONE = 1 if deg == 1 else (1, 0)

    def _c(self, v):
        return (v,) if self.deg == 1 else v

    def _u(self, cs):
        return cs[0] % self.Q if self.deg == 1 else (cs[0] % self.Q, cs[1] % self.Q)

    def add(self, a, b):
        return self._u([x + y for x, y in zip(self._c(a), self._c(b))])

    def sub(self, a, b):
        return self._u([x - y for x, y in zip(self._c(a), self._c(b))])

    def neg(self, a):
        return self.sub(self.ZERO, a)

    def mul(self, a, b):
        if self.deg == 1:
            return a * b % self.Q
        return ((a[0] * b[0] - a[1] * b[1]) % self.Q, (a[0] * b[1] + a[1] * b[0]) % self.Q)

    def inv(self, a):
        if self.deg == 1:
            return pow(a, -1, self.Q)
        n = pow(a[0] * a[0] + a[1] * a[1], -1, self.Q)
        return (a[0] * n % self.Q, -a[1] * n % self.Q)

    def rand(self, rng):
        return self._u([int.from_bytes(rng.bytes(48), "little") % (self.Q - 1) + 1 for _ in range(self.deg)])

    def lift(self, v, k):
        return np.concatenate([to_limbs(c * self.cfg.RP % self.Q + k * self.Q, self.L) for c in self._c(v)])

    def zero_limbs(self):
        return np.zeros(self.W, dtype=np.uint32)

    def decode(self, limbs):
        return self._u([from_limbs(limbs[h * self.L:(h + 1) * self.L]) * self.cfg.RP_INV for h in range(self.deg)])

    def closure(self, limbs):
        """the contract of every point routine's result: coordinates < 8q, limbs normalised"""
        for h in range(self.deg):
            c = limbs[h * self.L:(h + 1) * self.L]
            if from_limbs(c) >= 8 * self.Q or not (c[:self.L - 1] <= M28).all():
                return False
        return True

    def maxval(self, limbs):
        return max(from_limbs(limbs[h * self.L:(h + 1) * self.L]) for h in range(self.deg))


def _dbl_model(f, x, y, zz, zzz):
    """dbl-2008-s-1 (a = 0); with zz = zzz = 1: mdbl-2008-s-1"""
    u = f.add(y, y)
    v = f.mul(u, u)
    w = f.mul(u, v)
    s = f.mul(x, v)
    xx = f.mul(x, x)
    m = f.add(f.add(xx, xx), xx)
    x3 = f.sub(f.mul(m, m), f.add(s, s))
    y3 = f.sub(f.mul(m, f.sub(s, x3)), f.mul(w, y))
    return (x3, y3, f.mul(v, zz), f.mul(w, zzz))


def _add_model(f, p, q, mixed):
    """add-2008-s (madd-2008-s for zz2 = zzz2 = 1) on plain values, as rational functions: no curve equation is used.  Returns (branch class, XYZZ or None)."""
    p_inf, q_inf = p[2] == f.ZERO, q[2] == f.ZERO
    if q_inf:
        return ("both-infinity", None) if p_inf else ("right-infinity", p)
    if p_inf:
        return "left-infinity", q
    u1, u2 = f.mul(p[0], q[2]), f.mul(q[0], p[2])
    s1, s2 = f.mul(p[1], q[3]), f.mul(q[1], p[3])
    pp_, r = f.sub(u2, u1), f.sub(s2, s1)
    if pp_ == f.ZERO:
        if r == f.ZERO:
            return "doubling", (_dbl_model(f, *q) if mixed else _dbl_model(f, *p))  # the mixed addition doubles its affine operand
        return "cancel", None
    pp = f.mul(pp_, pp_)
    ppp = f.mul(pp_, pp)
    q_ = f.mul(u1, pp)
    x3 = f.sub(f.sub(f.mul(r, r), ppp), f.add(q_, q_))
    y3 = f.sub(f.mul(r, f.sub(q_, x3)), f.mul(s1, ppp))
    return "generic", (x3, y3, f.mul(f.mul(p[2], q[2]), pp), f.mul(f.mul(p[3], q[3]), ppp))


def _model(f, op, p, q):
    """expected (class, affine point or None) of one record of zl_test_point_op's ops on plain XYZZ values"""
    if op in (0, 1, 2):
        if op == 1:
            q = (q[0], f.neg(q[1]), q[2], q[3])
        cls, r = _add_model(f, p, q, op != 2)
    elif p[2] == f.ZERO and op != 4:
        cls, r = "infinity", None
    else:
        cls = "finite"
        r = _dbl_model(f, *p) if op == 3 else _dbl_model(f, p[0], p[1], f.ONE, f.ONE) if op == 4 else (p[0], f.neg(p[1]), p[2], p[3]) if op == 5 else p
    if r is None or r[2] == f.ZERO:
        return cls, None
    return cls, (f.mul(r[0], f.inv(r[2])), f.mul(r[1], f.inv(r[3])))


ADD_CLASSES = ("generic", "doubling", "cancel", "left-infinity", "right-infinity", "both-infinity")
HALF_CLASSES = ("u-agree-c0", "u-agree-c1", "pp0-r-agree-c0", "pp0-r-agree-c1")
LIFTS = [(7, 7, 7, 7), (0, 0, 0, 0), (7, 0, 7, 0), (3, 7, 1, 5)]


def _required_classes(group, op):
    if op in (0, 1):
        return ADD_CLASSES[:4] + (HALF_CLASSES if group == ZL_G2 else ())
    if op == 2:
        return ADD_CLASSES + (HALF_CLASSES if group == ZL_G2 else ())
    return ("finite",) if op == 4 else ("finite", "infinity")


def _embed(f, vals, lifts):
    return [f.zero_limbs() if v == f.ZERO and k is None else f.lift(v, k or 0) for v, k in zip(vals, lifts)]


@functools.lru_cache(maxsize=None)
def _point_records(curve_id, group, op):
    """Records of one (curve, group, op): list of (class, limbs (8, W), expected affine or None, bounds), interleaved so that every wave holds every class.
    Fixed seed.  On-curve expectations are the oracle's group law AND the restated formulas (asserted equal here, on the CPU); off-curve ones the formulas."""
    cfg, c, _ = CURVES[curve_id]
    f = _Field(cfg, 1 if group == ZL_G1 else 2)
    rng = np.random.Generator(np.random.PCG64(700 + 10 * group + op))
    if group == ZL_G1:
        add, G, mulp = po.g1_add, po.g1_generator(c), po.g1_mul
    else:
        add, G, mulp = po.g2_add, po.g2_generator(c), po.g2_mul
    neg = lambda P: None if P is None else (P[0], f.neg(P[1]))  # noqa: E731
    pts = [mulp(c, int(rng.integers(2, 1 << 40)), G) for _ in range(4)]
    by_class = {}

    def xyzz(P, z):
        if P is None:
            return (f.ONE, f.ONE, f.ZERO, f.ZERO)
        zz = f.mul(z, z)
        zzz = f.mul(zz, z)
        return (f.mul(P[0], zz), f.mul(P[1], zzz), zz, zzz)

    def emit(p, q, lp, lq, oracle, tag=None):
        cls, exp = _model(f, op, p, q)
        if oracle is not False:
            assert exp == oracle, (curve_id, group, op, cls)  # the restated formulas against the oracle's group law
        if tag is not None:
            assert cls == ("generic" if tag.startswith("u-") else "cancel"), (tag, cls)
            cls = tag
        lp = [None if (p[2] == f.ZERO and i >= 2) else k for i, k in enumerate(lp)]
        lq = [None if (q[2] == f.ZERO and i >= 2) else k for i, k in enumerate(lq)]
        limbs = np.stack(_embed(f, p, lp) + _embed(f, q, lq)).astype(np.uint32)
        by_class.setdefault(cls, []).append((cls, limbs, exp, (tuple(lp), tuple(lq))))

    INF = xyzz(None, None)
    pairs = []
    for i in range(len(pts)):
        P, Qn = pts[i], pts[(i + 1) % len(pts)]
        pairs += [(P, Qn), (P, P), (P, neg(P)), (None, Qn), (P, None), (None, None)]
    if op > 2:  # unary ops: every point once, and infinity
        pairs = [(P, None) for P in pts + [None]]
    for P, Qp in pairs:
        for lp in LIFTS:
            zp, zq = f.rand(rng), f.rand(rng)
            if op in (0, 1):  # mixed: q affine, canonical or in [q, 2q); q is never infinity
                if Qp is None:
                    continue
                for kq in (0, 1):
                    emit(xyzz(P, zp), (Qp[0], Qp[1], f.ONE, f.ONE), lp, (kq, kq, 0, 0), add(c, P, Qp if op == 0 else neg(Qp)))
            elif op == 2:
                emit(xyzz(P, zp), xyzz(Qp, zq), lp, lp[::-1], add(c, P, Qp))
            elif op == 4:  # dbl_affine: affine coordinates up to 8q, never infinity
                if P is not None:
                    emit((P[0], P[1], f.ONE, f.ONE), INF, (lp[0], lp[1], 0, 0), (0, 0, 0, 0), add(c, P, P))
            else:
                emit(xyzz(P, zp), INF, lp, (0, 0, 0, 0), add(c, P, P) if op == 3 else neg(P) if op == 5 else P)
    if group == ZL_G2 and op in (0, 1, 2):
        # off-curve: the formulas are rational functions of the coordinates.  u1 = x1 zz2, u2 = x2 zz1, s1 = y1 zzz2, s2 = y2 zzz1 are chosen, the coordinates follow.
        for tag in HALF_CLASSES:
            for lp in (LIFTS[0], LIFTS[1], LIFTS[3]):
                for _ in range(2):
                    zz1, zzz1, u1, s1, s2 = (f.rand(rng) for _ in range(5))
                    zz2, zzz2 = (f.rand(rng), f.rand(rng)) if op == 2 else (f.ONE, f.ONE)
                    d = f.rand(rng)
                    half = (0, d[1]) if tag.endswith("c0") else (d[0], 0)  # the difference lives in the OTHER component
                    if tag.startswith("u-"):
                        u2 = f.add(u1, half)
                    else:
                        u2, s2 = u1, f.add(s1, half)
                    y2 = f.mul(s2, f.inv(zzz1))
                    p = (f.mul(u1, f.inv(zz2)), f.mul(s1, f.inv(zzz2)), zz1, zzz1)
                    q = (f.mul(u2, f.inv(zz1)), f.neg(y2) if op == 1 else y2, zz2, zzz2)
                    emit(p, q, lp, lp[::-1] if op == 2 else (1, 0, 0, 0), False, tag)
    need = _required_classes(group, op)
    assert set(by_class) == set(need), (curve_id, group, op, sorted(by_class))  # every class non-empty, none unexpected
    recs = []
    while any(by_class.values()):  # round robin over the classes until the largest is spent
        for cls in need:
            if by_class[cls]:
                recs.append(by_class[cls].pop())
    if len(recs) % 8 == 0:  # a partial last wave in every form (8, 16 or 32 items per wave)
        recs.append(recs[0])
    assert len(recs) % 32 and len(recs) % 16 and len(recs) % 8
    first = {r[0] for r in recs[:8]}
    assert first >= set(need[:min(len(need), 8)]), (curve_id, group, op, first)  # already the first eight items (one wave of the octet form) hold every class
    return recs


def _check_point_records(run, curve_id, group, form_name, ops):
    cfg, _, _ = CURVES[curve_id]
    f = _Field(cfg, 1 if group == ZL_G1 else 2)
    for op in ops:
        recs = _point_records(curve_id, group, op)
        out = run(op, np.stack([r[1] for r in recs]))
        counts = {}
        for (cls, _, exp, bounds), o in zip(recs, out):
            info = (curve_id, "G1" if group == ZL_G1 else "G2", form_name, "op", op, cls, "lifts", bounds)
            assert all(f.closure(o[k]) for k in range(4)), info
            zz = f.decode(o[2])
            got = None if zz == f.ZERO else (f.mul(f.decode(o[0]), f.inv(zz)), f.mul(f.decode(o[1]), f.inv(f.decode(o[3]))))
            assert got == exp, info
            if op == 6 and exp is not None:
                assert f.maxval(o[0]) < f.Q and f.maxval(o[1]) < f.Q, info
            counts[cls] = counts.get(cls, 0) + 1
        for cls in _required_classes(group, op):  # a condition, not a measurement: every branch class was run and compared
            assert counts.get(cls, 0) > 0, (curve_id, group, form_name, op, cls)


def _form_runner(be, cid, group, form):
    return lambda op, arr: hook_point_form_op(be, cid, group, form, op, arr)


# ---- without a GPU: the generator's coverage and the model, against the host path of the scalar forms ---------------------------------
@pytest.mark.parametrize("curve_id", CURVE_IDS)
def test_generator_meets_the_branch_class_counts(curve_id):
    for group in (ZL_G1, ZL_G2):
        for op in range(7):
            recs = _point_records(curve_id, group, op)
            classes = [r[0] for r in recs]
            for cls in _required_classes(group, op):
                assert classes.count(cls) >= (3 if op < 3 else 1), (curve_id, group, op, cls)
            assert len(recs) % 8 and len(recs) % 16 and len(recs) % 32
    cfg = CURVES[curve_id][0]
    recs = _field_product_records(cfg)
    Q = cfg.Q
    muls = [r[1] for r in recs if r[0] == 0]
    assert any(b[1] == 0 and max(a) == 16 * Q for a, b in muls) and any(b[1] == 16 * Q and a == (16 * Q, 16 * Q) for a, b in muls)
    assert any(a[0] == a[1] == 16 * Q for a, _ in muls)
    sqrs = [r[1][0] for r in recs if r[0] == 1]
    assert (0, 16 * Q) in sqrs and (16 * Q, 0) in sqrs and (16 * Q, 16 * Q) in sqrs
    rows, first, second = _layout(list(range(45)))
    assert (second - first) % 32 == 19 and len(rows) % 32


@pytest.mark.parametrize("curve_id", CURVE_IDS)
def test_fq2_product_model_against_the_host_field(curve_id):
    """the Fq2 Montgomery product the GPU test expects, composed from host calls of the base field: c1 = muladd(a0, b1, a1, b0), c0 = muladd(a0, b0, a1, 32q - b1),
    and for a0 = a1 (b1 < 8q) also op 19: a (b0 - 0 + 16q) + (16q - b1) a"""
    cfg = CURVES[curve_id][0]
    Q = cfg.Q
    recs = [r for r in _field_product_records(cfg) if r[0] in (0, 1)]
    pairs = [(r[1][0], r[1][1] if r[0] == 0 else r[1][0]) for r in recs]

    def host(op, rows):
        arr = np.zeros((len(rows), 4, cfg.L), dtype=np.uint32)
        for i, row in enumerate(rows):
            for j, v in enumerate(row):
                arr[i, j] = to_limbs(v, cfg.L)
        return [from_limbs(o) for o in hook_fp28_op(None, op, arr, bn254=cfg.bn254)]

    c1 = host(2, [(a[0], b[1], a[1], b[0]) for a, b in pairs])
    c0 = host(2, [(a[0], b[0], a[1], 32 * Q - b[1]) for a, b in pairs])
    for (a, b), v0, v1 in zip(pairs, c0, c1):
        assert v0 < 2 * Q and v1 < 2 * Q and (v0 % Q, v1 % Q) == _mont_mul2(cfg, a, b)
    same = [(a, b) for a, b in pairs if a[0] == a[1] and a[0] <= 10 * Q and b[1] < 8 * Q and b[0] <= 2 * Q]
    assert same
    for (a, b), v in zip(same, host(19, [(a[0], b[0], 0, b[1]) for a, b in same])):
        assert v % Q == _mont_mul2(cfg, a, b)[0]


@pytest.mark.parametrize("group,hot", [(ZL_G1, False), (ZL_G2, False), (ZL_G2, True)], ids=["g1", "g2-called", "g2-inlined"])
def test_point_model_against_scalar_forms_host_bls12_381(group, hot):
    _check_point_records(lambda op, arr: hook_point_op(None, group, hot, op, arr), "bls12_381", group, "scalar-hot" if hot else "scalar", range(7))


@pytest.mark.parametrize("group,form", [(ZL_G1, FORM_SCALAR), (ZL_G2, FORM_SCALAR), (ZL_G2, FORM_SCALAR_HOT)], ids=["g1", "g2-called", "g2-inlined"])
def test_point_model_against_scalar_forms_host_bn254(group, form):
    _check_point_records(_form_runner(None, ZL_BN254, group, form), "bn254", group, "scalar-hot" if form == FORM_SCALAR_HOT else "scalar", range(7))


def test_new_hook_host_path_equals_the_existing_hook():
    """zl_test_point_form_op's scalar forms are zl_test_point_op's code: same limbs out, BLS12-381, host path"""
    for group, hot in ((ZL_G1, False), (ZL_G2, False), (ZL_G2, True)):
        arr = np.stack([r[1] for r in _point_records("bls12_381", group, 2)])
        assert (hook_point_form_op(None, ZL_BLS12_381, group, FORM_SCALAR_HOT if hot else FORM_SCALAR, 2, arr) == hook_point_op(None, group, hot, 2, arr)).all()


# ---- on the device ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("curve_id", CURVE_IDS)
def test_fp2pair_field_at_contract_bounds(backend, curve_id):
    cfg, _, cid = CURVES[curve_id]
    _check_pair_field(backend, cfg, cid)


@pytest.mark.gpu
@pytest.mark.parametrize("curve_id", CURVE_IDS)
def test_quad_point_addition_at_bounds(backend, curve_id):
    _check_point_records(_form_runner(backend, CURVES[curve_id][2], ZL_G1, FORM_QUAD), curve_id, ZL_G1, "quad", range(7))


@pytest.mark.gpu
@pytest.mark.parametrize("curve_id", CURVE_IDS)
@pytest.mark.parametrize("form", [FORM_PAIR, FORM_OCTET], ids=["pair", "octet"])
def test_pair_point_formulas_at_bounds(backend, curve_id, form):
    _check_point_records(_form_runner(backend, CURVES[curve_id][2], ZL_G2, form), curve_id, ZL_G2, "pair" if form == FORM_PAIR else "octet", range(6))


@pytest.mark.gpu
@pytest.mark.parametrize("group,form", [(ZL_G1, FORM_SCALAR), (ZL_G2, FORM_SCALAR), (ZL_G2, FORM_SCALAR_HOT)], ids=["g1", "g2-called", "g2-inlined"])
def test_bn254_scalar_point_formulas_at_bounds_device(backend, group, form):
    _check_point_records(_form_runner(backend, ZL_BN254, group, form), "bn254", group, "scalar-hot" if form == FORM_SCALAR_HOT else "scalar", range(7))
