"""Independent Python builder of the scalar-multiplication circuit (zl_circuit_ed_scalar_mul, include/zl_backend_ext.h) on top of the oracle's R1CS and LC,
the Boolean and select rows of tests/merkle_circuit_util.py and the curve constants of tests/edwards_util.py.  It pins what the header states: the allocation
order (s, the bits, the two first selects, then 5 + 6 + 2 records a step) and the rows
    quotient   A = divisor,  B = out,  C = dividend            (the compiler's mul_equals)
    double     xy, xx, yy;  (a xx + yy) x3 = 2 xy;  (2 - a xx - yy) y3 = yy - a xx
    add        u = (y1 - a x1)(x2 + y2), v0 = x1 y2, v1 = x2 y1, w = v0 v1;  (1 + d w) x3 = v0 + v1;  (1 - d w) y3 = u + a v0 - v1
Values come from Python integers and modular inverses; Q, the expected result, from edwards_util.mul -- another algorithm (extended coordinates from the top
bit)."""
import edwards_util as eu
import merkle_circuit_util as mu
from oracle_lib import po


def shape(bits: int):
    """(n_constraints, n_instance, n_witness)"""
    return 14 * bits - 8, 5, 14 * bits - 10


def full_bits(curve) -> int:
    return eu.params(curve)[3].bit_length()


def _quotient(cs, den: po.LC, num: po.LC) -> po.LC:
    p = cs.f.p
    out = cs.new_witness(cs.value(num) * pow(cs.value(den), -1, p))
    cs.enforce(den, out, num)
    return out


def _neg(lc: po.LC, p: int) -> po.LC:
    return lc.scale(p - 1, p)


def double(cs, a: int, pt):
    p = cs.f.p
    x, y = pt
    xy, xx, yy = cs.mul(x, y), cs.mul(x, x), cs.mul(y, y)
    axx = xx.scale(a, p)
    x3 = _quotient(cs, axx.add(yy, p), xy.add(xy, p))
    y3 = _quotient(cs, po.LC.const(2).add(_neg(axx, p), p).add(_neg(yy, p), p), yy.add(_neg(axx, p), p))
    return x3, y3


def add(cs, a: int, d: int, p1, p2):
    p = cs.f.p
    (x1, y1), (x2, y2) = p1, p2
    u = cs.mul(y1.add(_neg(x1.scale(a, p), p), p), x2.add(y2, p))
    v0, v1 = cs.mul(x1, y2), cs.mul(x2, y1)
    w = cs.mul(v0, v1)
    dw = w.scale(d, p)
    x3 = _quotient(cs, po.LC.const(1).add(dw, p), v0.add(v1, p))
    y3 = _quotient(cs, po.LC.const(1).add(_neg(dw, p), p), u.add(v0.scale(a, p), p).add(_neg(v1, p), p))
    return x3, y3


def scalar_mul_circuit(curve, bits: int, point, scalar: int, q=None, bit_values=None) -> po.R1CS:
    """q: the public result (default: the model's product); bit_values: the values of the Boolean witnesses (default: the bits of scalar) -- both for negative
    tests.  The records follow the bit VALUES, as a prover's would."""
    fq, a, d, l = eu.params(curve)
    assert 1 <= bits <= l.bit_length() and 0 <= scalar < min(l, 1 << bits)
    cs = po.R1CS(curve.fr)
    p = cs.f.p
    px, py = cs.new_public(point[0]), cs.new_public(point[1])
    qv = eu.mul(curve, scalar, point) if q is None else q
    qx, qy = cs.new_public(qv[0]), cs.new_public(qv[1])
    s = cs.new_witness(scalar)
    vals = [(scalar >> i) & 1 for i in range(bits)] if bit_values is None else list(bit_values)
    b = [mu.new_boolean_witness(cs, v) for v in vals]
    total = po.LC()
    for i, bi in enumerate(b):
        total = total.add(bi.scale(1 << i, p), p)
    cs.enforce(total, po.LC.const(1), s)
    r = (mu.select(cs, b[0], px, po.LC()), mu.select(cs, b[0], py, po.LC.const(1)))
    m = (px, py)
    for i in range(1, bits):
        m = double(cs, a, m)
        t = add(cs, a, d, r, m)
        r = (mu.select(cs, b[i], t[0], r[0]), mu.select(cs, b[i], t[1], r[1]))
    cs.enforce(r[0], po.LC.const(1), qx)
    cs.enforce(r[1], po.LC.const(1), qy)
    assert (cs.n_constraints, cs.n_instance, cs.n_witness) == shape(bits)
    return cs
