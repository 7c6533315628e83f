// zl_edwards.h -- the two embedded twisted Edwards curves of the reference's arkworks plugin over this backend's scalar fields: ed_on_bls12_381 (Jubjub, over
// BLS12-381 Fr) and ed-on-bn254 (Baby Jubjub, over BN254 Fr); DESIGN.md 4.8.  a x^2 + y^2 = 1 + d x^2 y^2 over F_q, q = the pairing curve's r; subgroup order
// l, cofactor 8.  `a` is a square and `d` is not, so the unified addition law is COMPLETE: no exceptional case, no point at infinity, the identity is the
// ordinary point (0, 1).  Everything here is ZL_HD: the host mirror and the kernels of zl_edwards_dev.hip run the same text, so their results agree byte for byte.
//
// The constants are the published parameters of the two arkworks crates, derived from the fractions below with Python integers (tests/edwards_util.py derives
// them again); they are NOT compared with arkworks bytes -- the reference holds no vectors for these curves.
//
// Arithmetic: the lazily reduced 9 x 29-bit Fr of zl_field28r.h, everything kept as x R' (R' = 2^261) and only BOUNDED until the canonical store.  Extended
// coordinates (X, Y, Z, T), x = X / Z, y = Y / Z, T = X Y / Z; dbl-2008-hwcd and the unified add-2008-hwcd, templated on a in {+1, -1} so that the product by
// `a` is free or a sign.  Bounds in units of q (B(x)); a product is < 2, a loaded element is a product, a coordinate of every point is a product or loaded:
//   add:  A = X1 X2, B = Y1 Y2, D = Z1 Z2, C = d (T1 T2): < 2 each.  (X1 + Y1)(X2 + Y2): 4 * 4 = 16.  E = that - (A + B) + 8q (subtrahend < 4, bias 2^3 >= 4 + 2):
//         < 10.  F = D - C + 4q: < 6.  G = D + C: < 4.  H = B - a A: a = -1: B + A < 4; a = +1: B - A + 4q < 6.  Products E F = 60, G H <= 24, E H <= 60, F G = 24.
//   dbl:  A = X^2, B = Y^2, ZZ = Z^2, XY = X Y: < 2.  E = 2 XY: < 4 (a product in place of hwcd's (X + Y)^2 - A - B: this multiplier has no cheaper square, and the
//         subtraction it saves would have cost a bias of 8).  C = 2 ZZ: < 4.
//         a = +1: G = A + B < 4, H = A - B + 4q < 6, F = G - C + 8q < 12: E F = 48, G H = 24, E H = 24, F G = 48.
//         a = -1: D = -A makes H = -(A + B) negative, so ALL FOUR of E, F, G, H are negated -- every output is a product of two of them: E' = 2 X (-Y) with
//         -Y = 4q - Y < 4 (fat, it only feeds the product): < 4; G' = A - B + 4q < 6; H' = A + B < 4; F' = C + G' < 10: E' F' = 40, G' H' = 24, E' H' = 16, F' G' = 60.
//   on-curve: x^2, y^2, x^2 y^2, d (x^2 y^2): 4 products; both sides are sums below 6 and go through canon (< 128).
//   affine:   Z^(q - 2) by square-and-multiply (products of products: 4), x = X Z^-1, y = Y Z^-1, the canonical store's mul(x, 1): 2.
// The largest requirement, 60, is within MUL_BOUND of both fields (70 on BLS12-381, 169 on BN254); EdBounds asserts every line, and the bias exponents against KQ_MAX.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "zl_field28r.h"

namespace openzl {
namespace ed {

constexpr int WINDOW = 4, WINDOWS = 63, TABLE = 1 << WINDOW;  // 63 four-bit digits cover 252 bits: both l; a 16-entry table of the lane's own point, entry 0 = (0, 1)
constexpr int COORDS = 4, LIMBS = 9;
constexpr int POINT_WORDS = COORDS * LIMBS;                    // u32 words of one extended point
constexpr size_t TABLE_BYTES = (size_t)TABLE * POINT_WORDS * 4;  // 2304 B per lane
enum Status : uint8_t { ST_OK = 0, ST_RANGE = 1, ST_CURVE = 2, ST_SUBGROUP = 3, ST_SCALAR = 4 };

template <class FrP> struct Curve;
template <>
struct Curve<BLS12_381_Fr> {  // Jubjub: a = -1, d = -(10240 / 10241) mod q
    using P = BLS12_381_Fr29;
    static constexpr int A = -1;
    ZL_HD static constexpr uint32_t d(int i) { constexpr uint32_t v[8] = {0xd6343eb1u, 0x01065fd6u, 0x37579d26u, 0x292d7f6du, 0xe6bd7fd4u, 0xf5fd9207u, 0x4bfa2b48u, 0x2a9318e7u}; return v[i]; }
    ZL_HD static constexpr uint32_t l(int i) { constexpr uint32_t v[8] = {0xd6f72cb7u, 0xd0970e5eu, 0xccc81082u, 0xa6682093u, 0x01343b00u, 0x06673b01u, 0x6533afa9u, 0x0e7db4eau}; return v[i]; }
};
template <>
struct Curve<BN254_Fr> {  // Baby Jubjub: a = 1, d = 168696 / 168700 mod q
    using P = BN254_Fr29;
    static constexpr int A = 1;
    ZL_HD static constexpr uint32_t d(int i) { constexpr uint32_t v[8] = {0xfb281473u, 0x736c2b06u, 0x8e01a829u, 0x2498beeeu, 0xe7844661u, 0x7a5fd2deu, 0x821016c0u, 0x1575bd81u}; return v[i]; }
    ZL_HD static constexpr uint32_t l(int i) { constexpr uint32_t v[8] = {0x392126f1u, 0x677297dcu, 0x3920ee0au, 0xab3eedb8u, 0xd0302b0bu, 0x370a08b6u, 0x5c263405u, 0x060c89ceu}; return v[i]; }
};
constexpr uint64_t COFACTOR = 8;

template <class FrP> using El = Fr28<typename Curve<FrP>::P>;
template <class FrP>
struct Pt {
    El<FrP> X, Y, Z, T;
};

// ---- the bound argument of the header's comment, line by line
constexpr int ed_log2_up(int v) { return v <= 1 ? 0 : 1 + ed_log2_up((v + 1) / 2); }
constexpr int ed_bias(int subtrahend) { return ed_log2_up(subtrahend + 2); }  // subk: 2^j >= B(b) + 2
constexpr int ed_max(int a, int b) { return a > b ? a : b; }
template <class FrP>
struct EdBounds {
    using P = typename Curve<FrP>::P;
    static constexpr int A = Curve<FrP>::A;
    static constexpr int PROD = 2, SUM2 = 2 * PROD;
    // add
    static constexpr int ADD_J_E = ed_bias(SUM2), ADD_E = PROD + (1 << ADD_J_E);
    static constexpr int ADD_J_F = ed_bias(PROD), ADD_F = PROD + (1 << ADD_J_F);
    static constexpr int ADD_G = SUM2;
    static constexpr int ADD_J_H = ed_bias(PROD), ADD_H = A < 0 ? SUM2 : PROD + (1 << ADD_J_H);
    static constexpr int ADD_MUL = ed_max(ed_max(SUM2 * SUM2, ADD_E * ADD_F), ed_max(ed_max(ADD_G * ADD_H, ADD_E * ADD_H), ADD_F * ADD_G));
    // dbl
    static constexpr int DBL_J_NEG = ed_bias(PROD), DBL_NEGY = 1 << DBL_J_NEG;  // a = -1 only
    static constexpr int DBL_E = SUM2, DBL_C = SUM2;
    static constexpr int DBL_J_D = ed_bias(PROD), DBL_DIFF = PROD + (1 << DBL_J_D);  // A - B
    static constexpr int DBL_J_F = ed_bias(DBL_C);                                    // a = +1 only: G - C
    static constexpr int DBL_G = A < 0 ? DBL_DIFF : SUM2, DBL_H = A < 0 ? SUM2 : DBL_DIFF;
    static constexpr int DBL_F = A < 0 ? DBL_C + DBL_G : SUM2 + (1 << DBL_J_F);
    static constexpr int DBL_MUL = ed_max(ed_max(A < 0 ? PROD * DBL_NEGY : PROD * PROD, DBL_E * DBL_F), ed_max(ed_max(DBL_G * DBL_H, DBL_E * DBL_H), DBL_F * DBL_G));
    // on-curve test and identity test: what canon sees
    static constexpr int CANON = ed_max(PROD + (1 << ed_bias(PROD)), SUM2);
    // the assignment trace (trace_item): u = (y1 - a x1)(x2 + y2) from loaded affine values, every other record a product of two of them
    static constexpr int TRACE_J_U = ed_bias(PROD), TRACE_U_LEFT = A < 0 ? SUM2 : PROD + (1 << TRACE_J_U);  // a = +1 only: y1 - x1
    static constexpr int TRACE_MUL = ed_max(TRACE_U_LEFT * SUM2, PROD * PROD);
    static constexpr int MAX_MUL = ed_max(ed_max(ADD_MUL, DBL_MUL), TRACE_MUL);
    static constexpr int MAX_J = ed_max(ed_max(ed_max(ADD_J_E, ADD_J_F), TRACE_J_U), ed_max(ed_max(ADD_J_H, DBL_J_NEG), ed_max(DBL_J_D, DBL_J_F)));
    static_assert(MAX_MUL <= P::MUL_BOUND, "a bound product above what mul takes");
    static_assert(MAX_J <= P::KQ_MAX, "subk: the table holds every bias");
    static_assert(CANON <= 128 && DBL_F <= 128 && ADD_E <= 128, "canon and the carried sums stay below 128 q");
};
static_assert(EdBounds<BLS12_381_Fr>::ADD_MUL == 60 && EdBounds<BLS12_381_Fr>::DBL_MUL == 60 && EdBounds<BLS12_381_Fr>::MAX_J == 3, "Jubjub: 60 of 70");
static_assert(EdBounds<BN254_Fr>::ADD_MUL == 60 && EdBounds<BN254_Fr>::DBL_MUL == 48 && EdBounds<BN254_Fr>::MAX_J == 3, "Baby Jubjub: 60 of 169");
static_assert(EdBounds<BLS12_381_Fr>::TRACE_MUL == 16 && EdBounds<BN254_Fr>::TRACE_MUL == 24, "the assignment trace: 16 and 24, below the group law's 60");

// ---- elements
template <class FrP>
ZL_HD El<FrP> from_words(const uint32_t* c) {  // 8 x 32-bit words of a value < 2^256 -> x R' (a product: < 2q)
    using P = typename Curve<FrP>::P;
    uint32_t rp[8];
    for (int k = 0; k < 8; k++) rp[k] = P::rp2(k);
    return zl::mul(zl::unpack28r<P>(c), zl::unpack28r<P>(rp));
}
template <class FrP>
ZL_HD El<FrP> small(uint32_t v) {
    uint32_t c[8] = {v, 0, 0, 0, 0, 0, 0, 0};
    return from_words<FrP>(c);
}
template <class FrP>
ZL_HD El<FrP> coeff_d() {
    uint32_t c[8];
    for (int k = 0; k < 8; k++) c[k] = Curve<FrP>::d(k);
    return from_words<FrP>(c);
}
// canonical u64 words -> element; false when the value is not below q
template <class FrP>
ZL_HD bool load(const uint64_t* w, El<FrP>& out) {
    uint32_t c[8];
    for (int i = 0; i < 4; i++) { c[2 * i] = (uint32_t)w[i]; c[2 * i + 1] = (uint32_t)(w[i] >> 32); }
    uint64_t br = 0;
    for (int i = 0; i < 8; i++) br = (((uint64_t)c[i] - FrP::mod(i) - br) >> 32) & 1;
    out = from_words<FrP>(c);
    return br != 0;
}
template <class FrP>
ZL_HD void store(uint64_t* w, const El<FrP>& m) {
    using P = typename Curve<FrP>::P;
    uint32_t o[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    const El<FrP> c = zl::canon(zl::mul(m, zl::unpack28r<P>(o)));
    uint32_t v[8];
    zl::pack28r<P>(v, c);
    for (int i = 0; i < 4; i++) w[i] = (uint64_t)v[2 * i] | ((uint64_t)v[2 * i + 1] << 32);
}
template <class FrP>
ZL_HD bool scalar_ok(const uint64_t* k) {  // below l
    uint64_t br = 0;
    for (int i = 0; i < 8; i++) {
        const uint32_t w = (uint32_t)(k[i >> 1] >> (32 * (i & 1)));
        br = (((uint64_t)w - Curve<FrP>::l(i) - br) >> 32) & 1;
    }
    return br != 0;
}
template <class FrP, int J>
ZL_HD El<FrP> sub(const El<FrP>& a, const El<FrP>& b) {  // a - b + 2^J q, carried
    using P = typename Curve<FrP>::P;
    uint32_t K[P::L];
    for (int i = 0; i < P::L; i++) K[i] = P::kq(J, i);
    return zl::subk(a, b, K);
}
template <class FrP>
ZL_HD bool is_zero(const El<FrP>& a) {  // a < 128 q
    const El<FrP> c = zl::canon(a);
    uint32_t o = 0;
    for (int i = 0; i < El<FrP>::L; i++) o |= c.l[i];
    return o == 0;
}

// ---- points
template <class FrP>
ZL_HD Pt<FrP> identity() {
    Pt<FrP> p;
    p.Y = p.Z = small<FrP>(1);
    for (int i = 0; i < El<FrP>::L; i++) p.X.l[i] = p.T.l[i] = 0;
    return p;
}
template <class FrP>
ZL_HD Pt<FrP> from_affine(const El<FrP>& x, const El<FrP>& y) {
    Pt<FrP> p;
    p.X = x;
    p.Y = y;
    p.Z = small<FrP>(1);
    p.T = zl::mul(x, y);
    return p;
}
template <class FrP>
ZL_HD bool on_curve(const El<FrP>& x, const El<FrP>& y) {
    using B = EdBounds<FrP>;
    const El<FrP> xx = zl::mul(x, x), yy = zl::mul(y, y), dt = zl::mul(coeff_d<FrP>(), zl::mul(xx, yy));
    El<FrP> lhs;
    if constexpr (B::A < 0) lhs = sub<FrP, ed_bias(B::PROD)>(yy, xx);
    else lhs = zl::add(xx, yy);
    const El<FrP> rhs = zl::add(small<FrP>(1), dt);
    return is_zero<FrP>(sub<FrP, ed_bias(B::SUM2)>(lhs, rhs));  // < 6 + 8
}
static_assert(6 + 8 <= 128, "the on-curve difference is within canon");
template <class FrP>
ZL_HD bool is_identity(const Pt<FrP>& p) {  // X = 0 and Y = Z
    return is_zero<FrP>(p.X) && is_zero<FrP>(sub<FrP, ed_bias(EdBounds<FrP>::PROD)>(p.Y, p.Z));
}
// unified, complete: P + Q for ANY two points of the curve (P = Q and the identity included)
template <class FrP>
ZL_HD Pt<FrP> add(const Pt<FrP>& p, const Pt<FrP>& q, const El<FrP>& d) {
    using B = EdBounds<FrP>;
    const El<FrP> a = zl::mul(p.X, q.X), b = zl::mul(p.Y, q.Y), c = zl::mul(d, zl::mul(p.T, q.T)), dd = zl::mul(p.Z, q.Z);
    const El<FrP> ab = zl::add(a, b);
    const El<FrP> e = sub<FrP, B::ADD_J_E>(zl::mul(zl::add(p.X, p.Y), zl::add(q.X, q.Y)), ab);
    const El<FrP> f = sub<FrP, B::ADD_J_F>(dd, c), g = zl::add(dd, c);
    El<FrP> h;
    if constexpr (B::A < 0) h = ab;
    else h = sub<FrP, B::ADD_J_H>(b, a);
    Pt<FrP> r;
    r.X = zl::mul(e, f);
    r.Y = zl::mul(g, h);
    r.T = zl::mul(e, h);
    r.Z = zl::mul(f, g);
    return r;
}
// P + (x, y) for an affine point handed over as x, y and d x y (the fixed-base table's entries; Z2 = 1): add without the product Z1 Z2 and with C = T1 (d x y).
// x, y and d x y are products (< 2) and D = Z1 is a coordinate (< 2), so every bound is add's.
template <class FrP>
ZL_HD Pt<FrP> madd(const Pt<FrP>& p, const El<FrP>& x, const El<FrP>& y, const El<FrP>& dxy) {
    using B = EdBounds<FrP>;
    const El<FrP> a = zl::mul(p.X, x), b = zl::mul(p.Y, y), c = zl::mul(p.T, dxy);
    const El<FrP> ab = zl::add(a, b);
    const El<FrP> e = sub<FrP, B::ADD_J_E>(zl::mul(zl::add(p.X, p.Y), zl::add(x, y)), ab);
    const El<FrP> f = sub<FrP, B::ADD_J_F>(p.Z, c), g = zl::add(p.Z, c);
    El<FrP> h;
    if constexpr (B::A < 0) h = ab;
    else h = sub<FrP, B::ADD_J_H>(b, a);
    Pt<FrP> r;
    r.X = zl::mul(e, f);
    r.Y = zl::mul(g, h);
    r.T = zl::mul(e, h);
    r.Z = zl::mul(f, g);
    return r;
}
// 2 P; p.T is not read, and r.T is only computed when want_t (the doublings in front of another doubling leave it out)
template <class FrP>
ZL_HD Pt<FrP> dbl(const Pt<FrP>& p, bool want_t) {
    using B = EdBounds<FrP>;
    using P = typename Curve<FrP>::P;
    const El<FrP> a = zl::mul(p.X, p.X), b = zl::mul(p.Y, p.Y), zz = zl::mul(p.Z, p.Z), c = zl::add(zz, zz);
    El<FrP> e, f, g, h;
    if constexpr (B::A < 0) {  // E, F, G, H all negated
        uint32_t K[P::L];
        El<FrP> zero;
        for (int i = 0; i < P::L; i++) { K[i] = P::kq(B::DBL_J_NEG, i); zero.l[i] = 0; }
        const El<FrP> xny = zl::mul(p.X, zl::subk_nc(zero, p.Y, K));
        e = zl::add(xny, xny);
        g = sub<FrP, B::DBL_J_D>(a, b);
        h = zl::add(a, b);
        f = zl::add(c, g);
    } else {
        const El<FrP> xy = zl::mul(p.X, p.Y);
        e = zl::add(xy, xy);
        g = zl::add(a, b);
        h = sub<FrP, B::DBL_J_D>(a, b);
        f = sub<FrP, B::DBL_J_F>(g, c);
    }
    Pt<FrP> r;
    r.X = zl::mul(e, f);
    r.Y = zl::mul(g, h);
    r.Z = zl::mul(f, g);
    if (want_t) r.T = zl::mul(e, h);
    else r.T = p.T;
    return r;
}
// z^(q - 2): 256 squarings of a running power that starts at one, a product by z at every set bit of the exponent
template <class FrP>
ZL_HD constexpr uint32_t qm2(int i) {
    uint64_t br = 2;
    uint32_t w = 0;
    for (int k = 0; k <= i; k++) {
        const uint64_t t = (uint64_t)FrP::mod(k) - br;
        w = (uint32_t)t;
        br = (t >> 32) & 1;
    }
    return w;
}
template <class FrP>
ZL_HD uint32_t qm2_word(int i) {
    constexpr uint32_t v[8] = {qm2<FrP>(0), qm2<FrP>(1), qm2<FrP>(2), qm2<FrP>(3), qm2<FrP>(4), qm2<FrP>(5), qm2<FrP>(6), qm2<FrP>(7)};
    return v[i];
}
template <class FrP>
ZL_HD El<FrP> inv(const El<FrP>& z) {
    El<FrP> r = small<FrP>(1);
#pragma unroll 1
    for (int i = 255; i >= 0; i--) {
        r = zl::mul(r, r);
        if ((qm2_word<FrP>(i >> 5) >> (i & 31)) & 1u) r = zl::mul(r, z);
    }
    return r;
}
template <class FrP>
ZL_HD void store_affine(uint64_t* out_xy, const Pt<FrP>& p) {
    const El<FrP> zi = inv<FrP>(p.Z);
    store<FrP>(out_xy, zl::mul(p.X, zi));
    store<FrP>(out_xy + 4, zl::mul(p.Y, zi));
}
ZL_HD void store_identity(uint64_t* out_xy) {
    for (int i = 0; i < 8; i++) out_xy[i] = i == 4 ? 1 : 0;
}

// ---- the windowed multiplication.  Tab: where the lane keeps its 16 multiples -- put(e, P), get(e) -- a local array on the host, the unit's scratch slot on the device.
template <class FrP, class Tab>
ZL_HD void build_table(Tab& tab, const Pt<FrP>& p, const El<FrP>& d) {
    tab.put(0, identity<FrP>());
    tab.put(1, p);
    Pt<FrP> cur = p;
#pragma unroll 1
    for (int e = 2; e < TABLE; e++) {  // e P = (e - 1) P + P: the unified law takes the doubling at e = 2 as well
        cur = add<FrP>(cur, p, d);
        tab.put(e, cur);
    }
}
ZL_HD uint32_t digit_of(const uint64_t* k, int w) { return (uint32_t)(k[w >> 4] >> (4 * (w & 15))) & 15u; }  // (read where the scalar lies: no indexed copy)
template <class FrP>
ZL_HD uint32_t l_digit(int w) {
    return (Curve<FrP>::l(w >> 3) >> (4 * (w & 7))) & 15u;
}
// k P from P's table: the low 252 bits of the scalar's four words, or k = l for a null pointer (the subgroup test)
template <class FrP, class Tab>
ZL_HD Pt<FrP> window_mul(const Tab& tab, const uint64_t* k8, const El<FrP>& d) {
    Pt<FrP> acc = tab.get(k8 ? digit_of(k8, WINDOWS - 1) : l_digit<FrP>(WINDOWS - 1));
#pragma unroll 1
    for (int w = WINDOWS - 2; w >= 0; w--) {
#pragma unroll 1
        for (int j = 0; j < WINDOW; j++) acc = dbl<FrP>(acc, j == WINDOW - 1);
        acc = add<FrP>(acc, tab.get(k8 ? digit_of(k8, w) : l_digit<FrP>(w)), d);
    }
    return acc;
}
// One item: out_xy = k P (canonical affine words) and 0, or (0, 1) and the LOWEST status code that applies.  Every item runs the same instructions whatever its
// status -- an out-of-range coordinate or a point off the curve is multiplied as it is (the field takes any 256-bit value within its bounds, the formulas have
// no exceptional case) and the result is discarded -- so a wave never diverges on untrusted data.
template <class FrP, class Tab>
ZL_HD uint8_t mul_item(const uint64_t* p_xy, const uint64_t* k, bool check_subgroup, Tab& tab, uint64_t* out_xy) {
    El<FrP> x, y;
    bool in_range = load<FrP>(p_xy, x);
    in_range &= load<FrP>(p_xy + 4, y);
    const bool curve_ok = on_curve<FrP>(x, y);
    const bool k_ok = scalar_ok<FrP>(k);
    const El<FrP> d = coeff_d<FrP>();
    build_table<FrP>(tab, from_affine<FrP>(x, y), d);
    bool sub_ok = true;
    Pt<FrP> r = identity<FrP>();
#pragma unroll 1
    for (int pass = check_subgroup ? 0 : 1; pass < 2; pass++) {  // one body of the window loop for l P and for k P (a scalar >= l is refused below)
        r = window_mul<FrP>(tab, pass ? k : nullptr, d);
        if (pass == 0) sub_ok = is_identity<FrP>(r);
    }
    const uint8_t st = !in_range ? ST_RANGE : !curve_ok ? ST_CURVE : !sub_ok ? ST_SUBGROUP : !k_ok ? ST_SCALAR : ST_OK;
    if (st == ST_OK) store_affine<FrP>(out_xy, r);
    else store_identity(out_xy);
    return st;
}
// ---- the complete assignment of zl_circuit_ed_scalar_mul (zl_host.h edwards::scalar_mul_le), one item: row = 14 bits - 5 elements of 4 canonical words,
//   [0] 1   [1..5) P.x P.y Q.x Q.y   [5] s   [6 .. 6 + bits) the bits   then R_1 = (select(b_0, P.x, 0), select(b_0, P.y, 1))   then per step i = 1 .. bits - 1
//   the 13 records   xy xx yy M.x M.y | u v0 v1 w T.x T.y | R.x R.y   of M_i = 2 M_{i-1} (M_0 = P), T = R_i + M_i, R_{i+1} = b_i ? T : R_i.
// Every record is an AFFINE coordinate or a product of affine coordinates; an inversion per group operation would cost 2 (bits - 1) Fermat ladders.  Instead:
//   pass 1  the ladder in extended coordinates (dbl, add, a select of registers by b_i); X, Y, Z of every M_i and T_i and the product of all Z in FRONT of each
//           are kept as raw limbs (x R', bounded, 9 words padded to 12) in the step's OWN 13 cells -- 8 elements of 48 B in 416 B; nothing else lives there yet;
//   one inversion of the product of all Z (skipped at bits = 1: no step);
//   pass 2  back down the steps (Montgomery's trick: Z^-1 = run * prefix, run *= Z): all 8 kept elements of a step are read before the step's M.x M.y T.x T.y
//           are stored in their cells, canonical;
//   pass 3  up again: the other 9 records of each step by plain products of the canonical affine values read back from those four cells (R_i is carried: it
//           is only known going up), the selects as copies of words.
// Bounds (units of q): a cell read back is loaded (a product: < 2); xy xx yy v0 v1 w: 2 * 2; x2 + y2 < 4; y1 - a x1: a = -1 a sum < 4, a = +1 a difference
// with bias 4 < 6: u at 6 * 4 = 24; pass 2's run * prefix, run * Z, X Z^-1 are products of products: EdBounds::TRACE_MUL.  Per step 19 + 12 + 18 products.
// An item with a coordinate >= q, a point off the curve or a scalar >= l or >= 2^bits returns false; its row is computed by the same instructions from
// whatever the operands are (no address depends on data) and is unspecified.
constexpr int STEP_RECORDS = 13, KEPT_WORDS64 = 6;  // a kept element: 9 limbs in 48 bytes
static_assert(8 * KEPT_WORDS64 <= STEP_RECORDS * 4, "the 8 kept elements of a step fit the step's 13 cells");
template <class FrP>
constexpr unsigned order_bits() {  // bit length of l: 252 (Jubjub), 251 (Baby Jubjub)
    unsigned n = 0;
    for (uint32_t top = Curve<FrP>::l(7); top; top >>= 1) n++;
    return 224 + n;
}
static_assert(order_bits<BLS12_381_Fr>() == 252 && order_bits<BN254_Fr>() == 251, "the scalar widths of the two curves");
constexpr size_t trace_row_elems(unsigned bits) { return 14 * (size_t)bits - 5; }
static_assert(trace_row_elems(252) == 3523 && trace_row_elems(251) == 3509, "n_instance + n_witness = 5 + (14 bits - 10); 3 520 and 3 506 rows at full width");
ZL_HD void put_cell(uint64_t* cell, uint64_t a, uint64_t b, uint64_t c, uint64_t d) {  // one element of canonical words; 16-byte aligned on the device
#ifdef __HIP_DEVICE_COMPILE__
    ulonglong2* q = reinterpret_cast<ulonglong2*>(cell);
    q[0] = make_ulonglong2(a, b);
    q[1] = make_ulonglong2(c, d);
#else
    cell[0] = a; cell[1] = b; cell[2] = c; cell[3] = d;
#endif
}
template <class FrP>
ZL_HD void put_elem(uint64_t* cell, const El<FrP>& m) {
    uint64_t w[4];
    store<FrP>(w, m);
    put_cell(cell, w[0], w[1], w[2], w[3]);
}
template <class FrP>
ZL_HD void keep(uint64_t* at, const El<FrP>& e) {  // raw limbs, as they are
    static_assert(El<FrP>::L == 9, "nine limbs in 48 bytes");
    put_cell(at, (uint64_t)e.l[0] | ((uint64_t)e.l[1] << 32), (uint64_t)e.l[2] | ((uint64_t)e.l[3] << 32), (uint64_t)e.l[4] | ((uint64_t)e.l[5] << 32),
             (uint64_t)e.l[6] | ((uint64_t)e.l[7] << 32));
    at[4] = e.l[8];
}
template <class FrP>
ZL_HD El<FrP> kept(const uint64_t* at) {
    El<FrP> e;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        e.l[2 * i] = (uint32_t)at[i];
        e.l[2 * i + 1] = (uint32_t)(at[i] >> 32);
    }
    e.l[8] = (uint32_t)at[4];
    return e;
}
ZL_HD bool scalar_bit(const uint64_t* k, unsigned i) { return (k[i >> 6] >> (i & 63)) & 1u; }
template <class FrP>
ZL_HD El<FrP> pick(bool take, const El<FrP>& a, const El<FrP>& b) {  // limb by limb: registers, never a copy through memory
    El<FrP> r;
#pragma unroll
    for (int i = 0; i < El<FrP>::L; i++) r.l[i] = take ? a.l[i] : b.l[i];
    return r;
}
template <class FrP>
ZL_HD Pt<FrP> pick(bool take, const Pt<FrP>& a, const Pt<FrP>& b) {
    return Pt<FrP>{pick<FrP>(take, a.X, b.X), pick<FrP>(take, a.Y, b.Y), pick<FrP>(take, a.Z, b.Z), pick<FrP>(take, a.T, b.T)};
}
// The ladder body of one multiplication k P: the cells of R_1 (sel0: 2 elements) and of the bits - 1 steps (13 elements each), written by the three passes
// above with one inversion; the kept elements live in the step's own cells.  x, y: P loaded; p_xy: its canonical words (copied into R_1 when b_0 is set).  The
// cells of the result -- the last select records, or R_1 when bits = 1 -- are ladder_result's.  Shared by zl_circuit_ed_scalar_mul's rows (trace_item) and the
// two ladders of zl_circuit_hybrid_encrypt's (hybrid_ladder_item).
template <class FrP>
ZL_HD void ladder_cells(const El<FrP>& x, const El<FrP>& y, const uint64_t* p_xy, const uint64_t* k, unsigned bits, uint64_t* sel0, uint64_t* steps) {
    using B = EdBounds<FrP>;
    const bool b0 = scalar_bit(k, 0);
    if (b0) {
        put_cell(sel0, p_xy[0], p_xy[1], p_xy[2], p_xy[3]);
        put_cell(sel0 + 4, p_xy[4], p_xy[5], p_xy[6], p_xy[7]);
    } else {
        put_cell(sel0, 0, 0, 0, 0);
        put_cell(sel0 + 4, 1, 0, 0, 0);
    }
    if (bits > 1) {
        const El<FrP> d = coeff_d<FrP>();
        // pass 1
        Pt<FrP> m = from_affine<FrP>(x, y), r = pick<FrP>(b0, m, identity<FrP>());
        El<FrP> pre = small<FrP>(1);
#pragma unroll 1
        for (unsigned i = 1; i < bits; i++) {
            uint64_t* at = steps + (size_t)(i - 1) * STEP_RECORDS * 4;
            m = dbl<FrP>(m, true);
            keep<FrP>(at, m.X);
            keep<FrP>(at + KEPT_WORDS64, m.Y);
            keep<FrP>(at + 2 * KEPT_WORDS64, m.Z);
            keep<FrP>(at + 3 * KEPT_WORDS64, pre);
            pre = zl::mul(pre, m.Z);
            const Pt<FrP> t = add<FrP>(r, m, d);
            keep<FrP>(at + 4 * KEPT_WORDS64, t.X);
            keep<FrP>(at + 5 * KEPT_WORDS64, t.Y);
            keep<FrP>(at + 6 * KEPT_WORDS64, t.Z);
            keep<FrP>(at + 7 * KEPT_WORDS64, pre);
            pre = zl::mul(pre, t.Z);
            r = pick<FrP>(scalar_bit(k, i), t, r);
        }
        El<FrP> run = inv<FrP>(pre);  // (no Z of an on-curve item is zero: the law is complete)
        // pass 2
#pragma unroll 1
        for (unsigned i = bits - 1; i >= 1; i--) {
            uint64_t* at = steps + (size_t)(i - 1) * STEP_RECORDS * 4;
            El<FrP> zi = zl::mul(run, kept<FrP>(at + 7 * KEPT_WORDS64));
            run = zl::mul(run, kept<FrP>(at + 6 * KEPT_WORDS64));
            const El<FrP> tx = zl::mul(kept<FrP>(at + 4 * KEPT_WORDS64), zi), ty = zl::mul(kept<FrP>(at + 5 * KEPT_WORDS64), zi);
            zi = zl::mul(run, kept<FrP>(at + 3 * KEPT_WORDS64));
            run = zl::mul(run, kept<FrP>(at + 2 * KEPT_WORDS64));
            const El<FrP> mx = zl::mul(kept<FrP>(at), zi), my = zl::mul(kept<FrP>(at + KEPT_WORDS64), zi);
            put_elem<FrP>(at + 3 * 4, mx);   // (every kept element of the step has been read)
            put_elem<FrP>(at + 4 * 4, my);
            put_elem<FrP>(at + 9 * 4, tx);
            put_elem<FrP>(at + 10 * 4, ty);
        }
        // pass 3
        El<FrP> px = x, py = y;  // M_{i-1} and R_i, affine
        El<FrP> rx = pick<FrP>(b0, x, identity<FrP>().X), ry = pick<FrP>(b0, y, small<FrP>(1));
        const uint64_t* sel = sel0;
#pragma unroll 1
        for (unsigned i = 1; i < bits; i++) {
            uint64_t* at = steps + (size_t)(i - 1) * STEP_RECORDS * 4;
            El<FrP> mx, my, tx, ty;
            (void)load<FrP>(at + 3 * 4, mx);
            (void)load<FrP>(at + 4 * 4, my);
            put_elem<FrP>(at, zl::mul(px, py));
            put_elem<FrP>(at + 4, zl::mul(px, px));
            put_elem<FrP>(at + 2 * 4, zl::mul(py, py));
            El<FrP> left;
            if constexpr (B::A < 0) left = zl::add(ry, rx);
            else left = sub<FrP, B::TRACE_J_U>(ry, rx);
            put_elem<FrP>(at + 5 * 4, zl::mul(left, zl::add(mx, my)));
            const El<FrP> v0 = zl::mul(rx, my), v1 = zl::mul(mx, ry);
            put_elem<FrP>(at + 6 * 4, v0);
            put_elem<FrP>(at + 7 * 4, v1);
            put_elem<FrP>(at + 8 * 4, zl::mul(v0, v1));
            (void)load<FrP>(at + 9 * 4, tx);  // (loaded whatever the bit: a wave does not diverge on the scalar)
            (void)load<FrP>(at + 10 * 4, ty);
            const bool take = scalar_bit(k, i);
            rx = pick<FrP>(take, tx, rx);
            ry = pick<FrP>(take, ty, ry);
            const uint64_t* from = take ? at + 9 * 4 : sel;
            put_cell(at + 11 * 4, from[0], from[1], from[2], from[3]);
            put_cell(at + 12 * 4, from[4], from[5], from[6], from[7]);
            sel = at + 11 * 4;
            px = mx;
            py = my;
        }
    }
}
ZL_HD const uint64_t* ladder_result(const uint64_t* sel0, const uint64_t* steps, unsigned bits) {  // 8 words: (x, y) of k P
    return bits > 1 ? steps + ((size_t)(bits - 2) * STEP_RECORDS + 11) * 4 : sel0;
}
ZL_HD bool scalar_fits(const uint64_t* k, unsigned bits) {  // below 2^bits
    bool ok = true;
#pragma unroll 1
    for (unsigned i = bits; i < 256; i++) ok &= !scalar_bit(k, i);
    return ok;
}
template <class FrP>
ZL_HD bool trace_item(const uint64_t* p_xy, const uint64_t* k, unsigned bits, uint64_t* row, uint64_t* q_out) {
    El<FrP> x, y;
    bool ok = load<FrP>(p_xy, x);
    ok &= load<FrP>(p_xy + 4, y);
    ok &= on_curve<FrP>(x, y);
    ok &= scalar_ok<FrP>(k);
#pragma unroll 1
    for (unsigned i = bits; i < 256; i++) ok &= !scalar_bit(k, i);
    uint64_t* bit_cells = row + 24;
    uint64_t* sel0 = bit_cells + (size_t)bits * 4;
    uint64_t* steps = sel0 + 8;
    put_cell(row, 1, 0, 0, 0);
    put_cell(row + 4, p_xy[0], p_xy[1], p_xy[2], p_xy[3]);
    put_cell(row + 8, p_xy[4], p_xy[5], p_xy[6], p_xy[7]);
    put_cell(row + 20, k[0], k[1], k[2], k[3]);
#pragma unroll 1
    for (unsigned i = 0; i < bits; i++) put_cell(bit_cells + (size_t)i * 4, scalar_bit(k, i) ? 1 : 0, 0, 0, 0);
    ladder_cells<FrP>(x, y, p_xy, k, bits, sel0, steps);
    const uint64_t* q = bits > 1 ? steps + ((size_t)(bits - 2) * STEP_RECORDS + 11) * 4 : sel0;
    uint64_t qw[8];
    for (int i = 0; i < 8; i++) qw[i] = q[i];
    put_cell(row + 12, qw[0], qw[1], qw[2], qw[3]);
    put_cell(row + 16, qw[4], qw[5], qw[6], qw[7]);
    if (q_out)
        for (int i = 0; i < 8; i++) q_out[i] = qw[i];
    return ok;
}

// ---- the complete assignment of zl_circuit_hybrid_encrypt (zl_host.hip hybrid_encrypt_circuit), its embedded-curve part.  T = N rate text elements, H header
// elements, L = 13 bits - 11 elements a ladder, S the cipher's recorded S-boxes at K = 2; row = 27 bits - 13 + 2 T + H + 3 S elements of 4 canonical words:
//   [0] 1   [1..3) G   [3..5) pk   [5..7) epk   [7] tag   [8 .. 8 + T) ciphertext   [.. + H) header   | esk   the bits   the G ladder (R_1, the steps)
//   the pk ladder in the same form   [.. + T) plaintext   then the 3 S records.
// One ITEM here is one (row, ladder), w the canonical words of the ladder's own point: ladder 0 multiplies G and also writes [0], G, pk, esk, the bit cells and epk (and epk_out, may be null); ladder 1
// multiplies pk and writes nothing outside its ladder's cells -- its result cells are S, which the cipher launch reads as its key.  The two items of a row
// touch disjoint cells and neither reads what the other writes, so they may run in any order or at once.  tag, ciphertext, header, plaintext and records are
// the cipher's to write (zl_poseidon_dev.h, DuplexRowLayout).  Ladder 0 answers for esk (below l and below 2^bits), ladder 1 for pk (coordinates below q, on
// the curve); G is the caller's to check, once per call.  No new arithmetic: every bound is trace_item's.
struct HybridRow {
    unsigned bits;
    size_t T, H, S;
    ZL_HD constexpr size_t ladder() const { return 13 * (size_t)bits - 11; }
    ZL_HD constexpr size_t esk_at() const { return 8 + T + H; }
    ZL_HD constexpr size_t bits_at() const { return esk_at() + 1; }
    ZL_HD constexpr size_t ladder_at(int which) const { return bits_at() + bits + (which ? ladder() : 0); }
    ZL_HD constexpr size_t plain_at() const { return ladder_at(1) + ladder(); }
    ZL_HD constexpr size_t key_at() const { return plain_at() - 2; }  // S = the pk ladder's result: its last two cells, the last select records or R_1
    ZL_HD constexpr size_t rec_at() const { return plain_at() + T; }
    ZL_HD constexpr size_t elems() const { return rec_at() + 3 * S; }
};
static_assert(HybridRow{1, 2, 0, 0}.elems() == 27 - 13 + 4 && HybridRow{252, 2, 0, 315}.elems() == 27 * 252 - 13 + 4 + 945, "27 bits - 13 + 2 T + H + 3 S");
static_assert(HybridRow{1, 2, 0, 0}.key_at() == HybridRow{1, 2, 0, 0}.ladder_at(1) &&
                  HybridRow{9, 2, 0, 0}.key_at() == HybridRow{9, 2, 0, 0}.ladder_at(1) + 2 + (9 - 2) * STEP_RECORDS + 11,
              "the key cells are R_1 at one bit, else ladder_result's: records 11 and 12 of the last step");
template <class FrP>
ZL_HD bool hybrid_ladder_item(const uint64_t* w, const uint64_t* pk_xy, const uint64_t* esk, const HybridRow& lay, int which, uint64_t* row, uint64_t* epk_out) {
    El<FrP> x, y;
    bool ok = load<FrP>(w, x);
    ok &= load<FrP>(w + 4, y);
    uint64_t* sel0 = row + lay.ladder_at(which) * 4;
    uint64_t* steps = sel0 + 8;
    if (which) {
        ok &= on_curve<FrP>(x, y);
    } else {
        ok = scalar_ok<FrP>(esk);  // (G was checked on the host)
        ok &= scalar_fits(esk, lay.bits);
        put_cell(row, 1, 0, 0, 0);
        put_cell(row + 4, w[0], w[1], w[2], w[3]);
        put_cell(row + 8, w[4], w[5], w[6], w[7]);
        put_cell(row + 12, pk_xy[0], pk_xy[1], pk_xy[2], pk_xy[3]);
        put_cell(row + 16, pk_xy[4], pk_xy[5], pk_xy[6], pk_xy[7]);
        put_cell(row + lay.esk_at() * 4, esk[0], esk[1], esk[2], esk[3]);
        uint64_t* bit_cells = row + lay.bits_at() * 4;
#pragma unroll 1
        for (unsigned i = 0; i < lay.bits; i++) put_cell(bit_cells + (size_t)i * 4, scalar_bit(esk, i) ? 1 : 0, 0, 0, 0);
    }
    ladder_cells<FrP>(x, y, w, esk, lay.bits, sel0, steps);
    if (!which) {
        const uint64_t* q = ladder_result(sel0, steps, lay.bits);
        uint64_t qw[8];
        for (int i = 0; i < 8; i++) qw[i] = q[i];
        put_cell(row + 20, qw[0], qw[1], qw[2], qw[3]);
        put_cell(row + 24, qw[4], qw[5], qw[6], qw[7]);
        if (epk_out)
            for (int i = 0; i < 8; i++) epk_out[i] = qw[i];
    }
    return ok;
}

// the host's table
template <class FrP>
struct LocalTab {
    Pt<FrP> t[TABLE];
    ZL_HD void put(int e, const Pt<FrP>& p) { t[e] = p; }
    ZL_HD Pt<FrP> get(int e) const { return t[e]; }
};
}  // namespace ed
}  // namespace openzl
