#!/usr/bin/env python3
"""Constants of the BN254 G2 endomorphism split (zl_params.h: BN254_GLS; kernel: zl_msm_endo.h k_gls_split_lattice) and a model of the kernel's integer
arithmetic that checks, on edge and random scalars, k0 + k1 lambda + k2 lambda^2 + k3 lambda^3 = k (mod r) and |k_j| < 2^QUARTER_BITS.

BN254: x = 4965661367192848881, r = 36x^4 + 36x^3 + 18x^2 + 6x + 1, q = 36x^4 + 36x^3 + 24x^2 + 6x + 1.  psi = twist . Frobenius . untwist acts on G2 as
[lambda], lambda = q mod r = 6x^2, a root of Phi_12: lambda^4 - lambda^2 + 1 = 0 (mod r) (Galbraith-Scott 2008).  psi(x, y) = (conj(x) gx, conj(y) gy) with
gx = xi^(+-(q-1)/3), gy = xi^(+-(q-1)/2), xi = 9 + u; the signs are found by checking psi(P) = [lambda]P with oracle/pyoracle.py.
Lattice L = {(a0..a3): sum a_j lambda^j = 0 mod r}, det r; b0..b3 = an LLL-reduced basis of it (computed here, exact rationals), then the unimodular neighbour
with the smallest largest column sum of |entries| (that sum is what bounds the quarters).  (k, 0, 0, 0) = sum_i w_i k b_i exactly, w = e0 B^-1; the kernel
rounds c_i = sign(w_i) ((k g_i + 2^255) >> 256), g_i = round(2^256 |w_i|), and returns (k, 0, 0, 0) - sum c_i b_i: a rounding off by one moves the result by one
basis row, which keeps the congruence exact.  |c_i - w_i k| <= 1/2 + k 2^-257 < 1/2 + 2^-3, so |k_j| <= (5/8) sum_i |b_i[j]|: the proved bound printed below.
"""
import itertools
import os
import random
import sys
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyoracle as po  # noqa: E402

x = 4965661367192848881
r = 36 * x**4 + 36 * x**3 + 18 * x**2 + 6 * x + 1
q = 36 * x**4 + 36 * x**3 + 24 * x**2 + 6 * x + 1
lam = q % r
assert r == po.BN254.fr.p and q == po.BN254.fq.p
assert lam == 6 * x * x and (lam**4 - lam**2 + 1) % r == 0
N_RANDOM = 400000
NW = 4  # words of the kernel's signed arithmetic (mod 2^128; sign = bit 127)


# ---- psi ---------------------------------------------------------------------------------------------------------------------------
def f2pow(a, e):
    res = (1, 0)
    while e:
        if e & 1:
            res = po.f2_mul(q, res, a)
        a = po.f2_mul(q, a, a)
        e >>= 1
    return res


def psi_apply(P, gx, gy):
    if P is None:
        return None
    (x0, x1), (y0, y1) = P
    return (po.f2_mul(q, (x0, (-x1) % q), gx), po.f2_mul(q, (y0, (-y1) % q), gy))


def psi_constants():
    c = po.BN254
    xi = (9, 1)
    P = po.g2_mul(c, 0x1234567, po.g2_generator(c))
    want = po.g2_mul(c, lam, P)
    found = []
    for sx, sy in itertools.product((1, -1), repeat=2):
        gx, gy = f2pow(xi, (q - 1) // 3), f2pow(xi, (q - 1) // 2)
        if sx < 0:
            gx = po.f2_inv(q, gx)
        if sy < 0:
            gy = po.f2_inv(q, gy)
        if psi_apply(P, gx, gy) == want:
            found.append((sx, sy, gx, gy))
    assert len(found) == 1, found
    return found[0]


# ---- lattice -----------------------------------------------------------------------------------------------------------------------
def dot(a, b):
    return sum(u * v for u, v in zip(a, b))


def lll(B, delta=Fraction(99, 100)):
    B = [list(v) for v in B]
    n = len(B)

    def gso():
        Bs, mu = [], [[Fraction(0)] * n for _ in range(n)]
        for i in range(n):
            v = [Fraction(t) for t in B[i]]
            for j in range(i):
                mu[i][j] = dot(B[i], Bs[j]) / dot(Bs[j], Bs[j])
                v = [a - mu[i][j] * b for a, b in zip(v, Bs[j])]
            Bs.append(v)
        return Bs, mu

    k = 1
    while k < n:
        for j in range(k - 1, -1, -1):
            _, mu = gso()
            m = round(mu[k][j])
            if m:
                B[k] = [a - m * b for a, b in zip(B[k], B[j])]
        Bs, mu = gso()
        if dot(Bs[k], Bs[k]) >= (delta - mu[k][k - 1] ** 2) * dot(Bs[k - 1], Bs[k - 1]):
            k += 1
        else:
            B[k], B[k - 1] = B[k - 1], B[k]
            k = max(k - 1, 1)
    return B


def det4(M):
    def det(m):
        if len(m) == 1:
            return m[0][0]
        return sum((-1) ** j * m[0][j] * det([row[:j] + row[j + 1:] for row in m[1:]]) for j in range(len(m)))
    return det([list(row) for row in M])


def colsum(B):
    return max(sum(abs(B[i][j]) for i in range(4)) for j in range(4))


def improve(B):
    """the unimodular neighbour (rows = combinations of the LLL rows with coefficients in {-1, 0, 1}) with the smallest largest column sum, the quantity that
    bounds |k_j|; ties go to the smaller total, then to the first found"""
    coefs = [c for c in itertools.product((-1, 0, 1), repeat=4) if any(c) and c > tuple(-t for t in c)]
    vecs = [[sum(c[i] * B[i][j] for i in range(4)) for j in range(4)] for c in coefs]
    absv = [[abs(t) for t in v] for v in vecs]
    best, best_key = None, None
    for idx in itertools.combinations(range(len(coefs)), 4):
        cols = [sum(absv[i][j] for i in idx) for j in range(4)]
        key = (max(cols), sum(cols))
        if best_key is not None and key >= best_key:
            continue
        if abs(det4([coefs[i] for i in idx])) != 1:
            continue
        best, best_key = [vecs[i] for i in idx], key
    return best


def basis():
    B0 = [[r, 0, 0, 0], [-lam, 1, 0, 0], [-(lam**2), 0, 1, 0], [-(lam**3), 0, 0, 1]]
    B = improve(lll(B0))
    for row in B:
        assert sum(a * lam**j for j, a in enumerate(row)) % r == 0, row
    d = det4(B)
    assert abs(d) == r, d
    return B, d


def in_x(v):
    """v as a polynomial in x with small coefficients, for the comment (checked)"""
    c1 = round(Fraction(v, x))
    c0 = v - c1 * x
    assert abs(c0) < 1000 and c1 * x + c0 == v
    if c1 == 0:
        return str(c0)
    t = ("-" if c1 < 0 else "") + ("" if abs(c1) == 1 else str(abs(c1))) + "x"
    return t if c0 == 0 else t + (" + " if c0 > 0 else " - ") + str(abs(c0))


B, DET = basis()
# w = e0 B^-1: w_i = cofactor(0, i) / det  (e0 = sum_i w_i b_i)
COF = []
for i in range(4):
    minor = [[B[a][b] for b in range(1, 4)] for a in range(4) if a != i]
    m = (minor[0][0] * (minor[1][1] * minor[2][2] - minor[1][2] * minor[2][1]) - minor[0][1] * (minor[1][0] * minor[2][2] - minor[1][2] * minor[2][0])
         + minor[0][2] * (minor[1][0] * minor[2][1] - minor[1][1] * minor[2][0]))
    COF.append((-1) ** i * m)
W = [Fraction(cf, DET) for cf in COF]
assert all(sum(W[i] * B[i][j] for i in range(4)) == (1 if j == 0 else 0) for j in range(4))
SG = [1 if w >= 0 else -1 for w in W]
G = [((abs(cf) << 256) + r // 2) // r for cf in COF]  # round(2^256 |w_i|)
NG = max((g.bit_length() + 31) // 32 for g in G)
NB = max((abs(v).bit_length() + 31) // 32 for row in B for v in row)
BOUND = Fraction(5, 8) * colsum(B)  # proved: |k_j| <= (1/2 + 2^-3) sum_i |b_i[j]|
QUARTER_BITS = 0
while BOUND >= (1 << QUARTER_BITS):
    QUARTER_BITS += 1
FILL_PCT = int(BOUND * 100 / (1 << QUARTER_BITS)) + 1  # the quarters stay below this share of 2^QUARTER_BITS
assert QUARTER_BITS + 2 <= 32 * NW - 1


def split_model(k):
    """the kernel's arithmetic: k reduced once, unsigned products on magnitudes, everything modulo 2^(32 NW), sign from the top bit"""
    M = 1 << (32 * NW)
    if k >= r:
        k -= r
    c = [((k * G[i] + (1 << 255)) >> 256) % M for i in range(4)]
    out = []
    for j in range(4):
        acc = (k if j == 0 else 0) % M
        for i in range(4):
            t = (c[i] * abs(B[i][j])) % M
            acc = (acc - t) % M if SG[i] * B[i][j] > 0 else (acc + t) % M
        out.append(acc - M if acc >> (32 * NW - 1) else acc)
    return out


def edge_scalars(mults=40):
    """0, 1, r - 1; multiples (1 .. mults - 1 and the last two below r) and neighbours of lambda, lambda^2, lambda^3 and of every basis entry; values in [r, 2^254)"""
    e = [0, 1, 2, r - 1, r - 2, (r - 1) // 2, (r + 1) // 2]
    for p in (lam, lam**2 % r, lam**3 % r):
        e += [(m * p + d) % r for m in list(range(1, mults)) + [r // p, r // p - 1] for d in (-1, 0, 1)]
    for v in sorted({abs(t) for row in B for t in row if t}):
        e += [(m * v + d) % r for m in list(range(1, mults)) + [r // v, r // v - 1] for d in (-1, 0, 1)]
        e += [r - v]
    e += [r, r + 1, r + lam, (1 << 254) - 1, (1 << 254) - lam, r + (1 << 200) + 12345]  # in [r, 2^254): reduced once
    return e


def words(v, n):
    return ", ".join("0x%08xu" % ((v >> (32 * i)) & 0xFFFFFFFF) for i in range(n))


def main():
    sx, sy, gx, gy = psi_constants()
    rnd = random.Random(1)
    edge = edge_scalars()
    worst = 0
    hist = [[0] * 32 for _ in range(4)]  # |k_j| of the random scalars over 32 equal parts of [0, 2^QUARTER_BITS)
    for n, k in enumerate(edge + [rnd.randrange(r) for _ in range(N_RANDOM)]):
        ks = split_model(k)
        assert (sum(kj * lam**j for j, kj in enumerate(ks)) - k) % r == 0, hex(k)
        worst = max(worst, max(abs(t) for t in ks))
        if n >= len(edge):
            for j, t in enumerate(ks):
                hist[j][(abs(t) << 5) >> QUARTER_BITS] += 1
    assert worst <= BOUND < (1 << QUARTER_BITS)
    # a full top window's busiest buckets against an even spread: the quarters crowd towards 0 (a sum of four roundings), far below what FILL_PCT alone allows
    peak_pct = max(max(h) for h in hist) * 32 * 100 // N_RANDOM
    R = 1 << 256
    sub = 0
    for i in range(4):
        for j in range(4):
            if SG[i] * B[i][j] > 0:
                sub |= 1 << (4 * i + j)
    print(f"// generated by tools/gen_bn254_gls.py (proved |k_j| <= {float(BOUND / (1 << 64)):.4f} * 2^64; worst over {len(edge) + N_RANDOM} scalars: {worst / (1 << 64):.4f} * 2^64)")
    print("struct BN254_GLS {")
    print("    static constexpr bool LATTICE = true;  // four-dimensional lattice split (k_gls_split_lattice)")
    print(f"    static constexpr int QUARTER_BITS = {QUARTER_BITS}, FILL_PCT = {FILL_PCT};  // |k_j| < 2^QUARTER_BITS, and below FILL_PCT % of it")
    print(f"    static constexpr int PEAK_PCT = {peak_pct};  // of {N_RANDOM} random scalars, the busiest 1/32 of [0, 2^QUARTER_BITS) holds PEAK_PCT % of an even share of the |k_j|")
    print(f"    static constexpr int NG = {NG}, NB = {NB};  // words of g_i and of |b_i[j]|")
    print(f"    // x = {x}, lambda = 6x^2; basis rows of {{a: sum a_j lambda^j = 0 mod r}}, det = {'+' if DET > 0 else '-'}r:")
    for i, row in enumerate(B):
        print(f"    //   b{i} = ({', '.join(in_x(v) for v in row)})")
    print("    // c_i = (k g_i + 2^255) >> 256, g_i = round(2^256 |w_i|), (1, 0, 0, 0) = sum w_i b_i")
    print("    ZL_HD static constexpr uint32_t g(int i, int w) {")
    print(f"        constexpr uint32_t v[4][{NG}] = {{{', '.join('{' + words(g, NG) + '}' for g in G)}}};")
    print("        return v[i][w];")
    print("    }")
    print("    ZL_HD static constexpr uint32_t b(int i, int j, int w) {  // |b_i[j]|")
    print(f"        constexpr uint32_t v[4][4][{NB}] = {{{', '.join('{' + ', '.join('{' + words(abs(t), NB) + '}' for t in row) + '}' for row in B)}}};")
    print("        return v[i][j][w];")
    print("    }")
    print(f"    static constexpr uint32_t SUB = 0x{sub:04x}u;  // bit 4 i + j: c_i |b_i[j]| is subtracted from quarter j (sign(w_i) b_i[j] > 0), else added")
    print(f"    ZL_HD static constexpr uint32_t rmod(int i) {{ constexpr uint32_t v[8] = {{{words(r, 8)}}}; return v[i]; }}  // the group order (scalars in [r, 2^254) are reduced once)")
    print(f"    // psi constants gx = xi^({'' if sx > 0 else '-'}(q-1)/3), gy = xi^({'' if sy > 0 else '-'}(q-1)/2), xi = 9 + u: Montgomery (R = 2^256), c0 then c1")
    for nm, v in (("psi_x0", gx[0]), ("psi_x1", gx[1]), ("psi_y0", gy[0]), ("psi_y1", gy[1])):
        print(f"    ZL_HD static constexpr uint32_t {nm}(int i) {{ constexpr uint32_t v[8] = {{{words(v * R % q, 8)}}}; return v[i]; }}")
    print("};")
    print(f"// lambda = {hex(lam)}; g bits {[g.bit_length() for g in G]}; signs of w {SG}; basis bits {[[abs(v).bit_length() for v in row] for row in B]}", file=sys.stderr)
    print(f"// QUARTER_BITS = {QUARTER_BITS}: proved bound {float(BOUND):.6e} = {float(BOUND / (1 << QUARTER_BITS)):.4f} * 2^{QUARTER_BITS}; observed {worst / (1 << QUARTER_BITS):.4f} * 2^{QUARTER_BITS}", file=sys.stderr)


if __name__ == "__main__":
    main()
