"""Python-integer model of the embedded twisted Edwards curves and the hybrid encryption (include/zl_backend_ext.h: zl_ed_*, zl_hybrid_*), independent of the
library.  a x^2 + y^2 = 1 + d x^2 y^2 over F_q, q = the pairing curve's r:
    BLS12-381 (Jubjub)       a = -1, d = -(10240 / 10241), l = 6554484396890773809930967563523245729705921265872317281365359162392183254199
    BN254 (Baby Jubjub)      a = 1,  d = 168696 / 168700,  l = 2736030358979909402780800718157159386076813972158567259200215660948447373041
the constants derived HERE from the two fractions; cofactor 8.  Extended coordinates with one inversion per result, plain double-and-add (not the library's
windows), the unified addition for everything.  Hybrid encryption on top of poseidon_duplex_util: the key is (x, y) of the affine shared secret."""
import functools

import numpy as np

import poseidon_duplex_util as du
import poseidon_util as pu

CURVES = pu.CURVES
COFACTOR = 8
ORDERS = {"bls12_381": 6554484396890773809930967563523245729705921265872317281365359162392183254199,
          "bn254": 2736030358979909402780800718157159386076813972158567259200215660948447373041}


@functools.lru_cache(maxsize=None)
def _params(q):
    if q.bit_length() == 255:
        return q - 1, (-(10240 * pow(10241, -1, q))) % q, ORDERS["bls12_381"]
    return 1, 168696 * pow(168700, -1, q) % q, ORDERS["bn254"]


def params(curve):
    """(q, a, d, l)"""
    q = curve.fr.p
    return (q,) + _params(q)


def is_square(v, q):
    return v % q == 0 or pow(v, (q - 1) // 2, q) == 1


def sqrt(v, q):
    """Tonelli-Shanks; None for a non-square"""
    v %= q
    if v == 0:
        return 0
    if not is_square(v, q):
        return None
    s, t = 0, q - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    z = 2
    while is_square(z, q):
        z += 1
    m, c, u, r = s, pow(z, t, q), pow(v, t, q), pow(v, (t + 1) // 2, q)
    while u != 1:
        i, w = 0, u
        while w != 1:
            w, i = w * w % q, i + 1
        b = pow(c, 1 << (m - i - 1), q)
        m, c, u, r = i, b * b % q, u * b * b % q, r * b % q
    return r


def on_curve(curve, p):
    q, a, d, _ = params(curve)
    x, y = p
    return (a * x * x + y * y - 1 - d * x * x * y * y) % q == 0


# ---- extended coordinates (X, Y, Z, T) ------------------------------------------------------------------------------------------------------------------
def _ext(p):
    return (p[0], p[1], 1, p[0] * p[1])


def _add(curve, p, r):
    q, a, d, _ = params(curve)
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = r
    A, B, C, D = x1 * x2 % q, y1 * y2 % q, d * t1 * t2 % q, z1 * z2 % q
    E = ((x1 + y1) * (x2 + y2) - A - B) % q
    F, G, H = (D - C) % q, (D + C) % q, (B - a * A) % q
    return (E * F % q, G * H % q, F * G % q, E * H % q)


def _affine(curve, p):
    q = curve.fr.p
    zi = pow(p[2], -1, q)
    return (p[0] * zi % q, p[1] * zi % q)


def add(curve, p, r):
    return _affine(curve, _add(curve, _ext(p), _ext(r)))


def mul(curve, k, p):
    """k p by double-and-add from the top bit, every step the unified addition"""
    acc, base = (0, 1, 1, 0), _ext(p)
    for bit in bin(k)[2:] if k else "":
        acc = _add(curve, acc, acc)
        if bit == "1":
            acc = _add(curve, acc, base)
    return _affine(curve, acc)


def random_points(curve, n, seed):
    """n points of the curve, anywhere in the full group (order 8 l): a random y, the x of the curve equation, a random sign"""
    q, a, d, _ = params(curve)
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        y = int.from_bytes(rng.bytes(40), "little") % q
        x = sqrt((1 - y * y) * pow(a - d * y * y, -1, q), q)
        if x is None:
            continue
        if rng.integers(2):
            x = (q - x) % q
        assert on_curve(curve, (x, y))
        out.append((x, y))
    return out


def subgroup_points(curve, n, seed):
    return [mul(curve, COFACTOR, p) for p in random_points(curve, n, seed)]


@functools.lru_cache(maxsize=None)
def _small(name):
    curve = {c.name: c for c in CURVES}[name]
    q, a, d, l = params(curve)
    o2 = (0, q - 1)
    o4 = (sqrt(pow(a, -1, q), q), 0)
    assert on_curve(curve, o4) and mul(curve, 2, o4) == o2
    for p in random_points(curve, 64, 4242):
        o8 = mul(curve, l, p)
        if mul(curve, 4, o8) == o2:
            return o2, o4, o8
    raise AssertionError("no point of order 8 among 64 random points")


def small_order_points(curve):
    """(a point of order 2, of order 4, of order 8)"""
    return _small(curve.name)


def random_scalars(curve, n, seed):
    l = params(curve)[3]
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "little") % l for _ in range(n)]


def edge_scalars(curve):
    """0, 1, 2, 15, 16, l - 1, 2^k and 2^k - 1 for k in {4, 64, 128, 248}, all-f nibbles, alternating nibbles"""
    l = params(curve)[3]
    out = [0, 1, 2, 15, 16, l - 1]
    for k in (4, 64, 128, 248):
        out += [1 << k, (1 << k) - 1]
    out += [(1 << 248) - 1, int("f0" * 31, 16), int("0f" * 31, 16), int("a5" * 31, 16)]
    assert all(v < l for v in out)
    return out


# ---- words ---------------------------------------------------------------------------------------------------------------------------------------------------
def point_words(points) -> np.ndarray:
    """[(x, y), ...] -> (count, 2, 4) uint64"""
    points = list(points)
    return pu.limbs([v for p in points for v in p]).reshape(len(points), 2, 4)


def points_of(words):
    v = pu.ints(np.asarray(words, dtype=np.uint64).reshape(-1, 4))
    return [(v[2 * i], v[2 * i + 1]) for i in range(len(v) // 2)]


# ---- hybrid encryption -------------------------------------------------------------------------------------------------------------------------------------
def hybrid_encrypt(curve, initial_state, generator, esk, pk, header, plaintext):
    """-> (epk, ciphertext blocks, tag): epk = esk G, the duplex cipher under the key (x, y) of esk pk"""
    s = mul(curve, esk, pk)
    ct, tag = du.encrypt(curve, initial_state, list(s), header, plaintext)
    return mul(curve, esk, generator), ct, tag


def hybrid_decrypt(curve, initial_state, sk, epk, header, ciphertext, tag):
    """-> (plaintext blocks, ok)"""
    s = mul(curve, sk, epk)
    return du.decrypt(curve, initial_state, list(s), header, ciphertext, tag)


# ---- the shared references of the tests: computed once, never changed ----------------------------------------------------------------------------------------
ID = (0, 1)
_REF = {}


def ref(curve):
    """the points and scalars of the multiplication tests and their model products, computed once per curve and never changed"""
    if curve.name not in _REF:
        o2, o4, o8 = small_order_points(curve)
        sub = subgroup_points(curve, 2, 11)
        pts = [ID, o2, o4, o8, add(curve, sub[0], o8), add(curve, sub[1], o2), sub[0]] + random_points(curve, 2, 12)
        ks = edge_scalars(curve) + random_scalars(curve, 6, 13)
        pairs = [(p, k) for p in pts for k in ks]
        _REF[curve.name] = (pts, ks, pairs, [mul(curve, k, p) for p, k in pairs])
        assert all(on_curve(curve, p) for p in pts)
    return _REF[curve.name]


SHAPES = [(3, 0, 1), (6, 3, 2)]
_HYB = {}


def hybrid_ref(curve, shape, count=6):
    """(state, G, esks, sks, pks, headers, plaintexts, model encryptions) of `count` messages, each to its own recipient; computed once"""
    key = (curve.name, shape)
    if key not in _HYB:
        width, h, n = shape
        rate = width - 1
        st = pu.random_elems(curve, width, 70 + width)
        g = subgroup_points(curve, 1, 71)[0]
        esks, sks = random_scalars(curve, count, 72), random_scalars(curve, count, 73)
        pks = [mul(curve, sk, g) for sk in sks]
        vals = pu.random_elems(curve, count * (h + n * rate), 74)
        headers = [vals[i * h:(i + 1) * h] for i in range(count)]
        tv = vals[count * h:]
        texts = [[tv[(i * n + j) * rate:(i * n + j + 1) * rate] for j in range(n)] for i in range(count)]
        enc = [hybrid_encrypt(curve, st, g, esks[i], pks[i], headers[i], texts[i]) for i in range(count)]
        _HYB[key] = (st, g, esks, sks, pks, headers, texts, enc)
    return _HYB[key]


def hybrid_words(curve, shape):
    width, h, n = shape
    st, g, esks, sks, pks, headers, texts, enc = hybrid_ref(curve, shape)
    count = len(esks)
    return dict(st=pu.limbs(st), g=point_words([g])[0], esk=pu.limbs(esks), sk=pu.limbs(sks), pk=point_words(pks),
                h=pu.limbs([v for hd in headers for v in hd]).reshape(count, h, 4), t=du.text_words(texts, width),
                epk=point_words([e[0] for e in enc]), ct=du.text_words([e[1] for e in enc], width), tag=pu.limbs([e[2] for e in enc]))
