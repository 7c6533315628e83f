// zl_decode.h -- decoding of arkworks-compressed G1 / G2 points (the format of zl_serialize.h) as lane-uniform code: the same templates run on the
// host (the test hook zl_test_decode_points_host) and, one lane per point, in the kernels of zl_decode_dev.hip.
//
// Statuses, their precedence and the outputs are those of serialize::Codec::g1_from_bytes / g2_from_bytes (zl_serialize.h), which stays the yardstick the
// tests compare against:
//   ZL_EINVAL     both flag bits, an x that is not a canonical integer < q, flag bits on the c0 half of a G2 x, the infinity flag with x != 0
//   ZL_ENOTCURVE  x^3 + b has no square root, or the point is outside the subgroup of order r
//   ZL_OK         xy = canonical affine words and inf = 0, or all-zero words and inf = 1
// and on every status but ZL_OK xy is all-zero and inf is 0.
//
// What differs from the host codec is the shape of the code, not the result.  A failing record changes what decode_* returns, never what it executes: there is
// no early return, an unusable x is replaced by the generator's and carried through the square root and the subgroup check, and the status is selected at the end.  The
// remaining branches are on constants (the bits of (q - 3) / 4 and of r, looked up per step in their constant tables by the loop counter), which every lane of a wave shares, and the exceptional cases inside the
// XYZZ formulas of zl_curve.h (infinity, equal or opposite operands), which points of order r meet only in the last addition.
//   fq_sqrt    q = 3 mod 4 on both curves: t = a^((q - 3) / 4) by one fixed-window power; a t is the candidate root and t its inverse
//              (a t^2 = a^((q - 1) / 2) = 1 for a non-zero square), which saves fq2_sqrt its inversion.
//   fq2_sqrt   u^2 = -1, through the norm like the host codec: s = sqrt(a0^2 + a1^2), x0 = sqrt((a0 + s) / 2) or sqrt((a0 - s) / 2), x1 = a1 / (2 x0).  Both
//              candidates are computed and one is selected.  a1 = 0 uses the same two roots on a0 and -a0: (sqrt(a0), 0) or (0, sqrt(-a0)).  Three powers.
//   in_subgroup  r P = infinity by double-and-add over the bits of r.  No endomorphism shortcut: a wrong one accepts forged points.
#pragma once
#include <stddef.h>
#include <type_traits>
#include "zl_curve.h"
#include "../../include/zl_backend.h"

namespace openzl {
namespace decode {

// (q - 3) / 4 as little-endian words: q = 3 mod 4, so the subtraction does not borrow
template <class P>
ZL_HD constexpr uint32_t sqrt_exp_word(int i) {
    static_assert((P::mod(0) & 3u) == 3u, "q = 3 mod 4");
    const uint32_t lo = i == 0 ? P::mod(0) - 3u : P::mod(i);
    const uint32_t hi = i + 1 < P::N ? P::mod(i + 1) : 0u;
    return (lo >> 2) | (hi << 30);
}
constexpr int SQRT_WINDOW = 3;  // 7 table entries: all of them stay in registers beside the accumulator (a 4-bit window would hold 15)

template <class P>
ZL_HD Fp<P> halve(const Fp<P>& a) {  // a / 2 (linear, so it holds in Montgomery form too): (a + (a odd ? q : 0)) >> 1; a + q < 2^(32 N)
    constexpr int N = P::N;
    const uint32_t mask = (uint32_t)0 - (a.l[0] & 1u);
    Fp<P> r;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        c += (uint64_t)a.l[i] + (P::mod(i) & mask);
        r.l[i] = (uint32_t)c;
        c >>= 32;
    }
#pragma unroll
    for (int i = 0; i < N; i++) r.l[i] = (r.l[i] >> 1) | (i + 1 < N ? r.l[i + 1] << 31 : 0u);
    return r;
}
template <class P>
ZL_HD Fp<P> select(bool c, const Fp<P>& a, const Fp<P>& b) {  // c ? a : b, limb by limb
    Fp<P> r;
#pragma unroll
    for (int i = 0; i < P::N; i++) r.l[i] = c ? a.l[i] : b.l[i];
    return r;
}
template <class P>
ZL_HD Fp2<P> select(bool c, const Fp2<P>& a, const Fp2<P>& b) { return Fp2<P>{select(c, a.c0, b.c0), select(c, a.c1, b.c1)}; }

// t = a^((q - 3) / 4): SQRT_WINDOW-bit windows from the top.  The loop is not unrolled, so a digit is a lookup in the constant table of the exponent's words by
// the loop counter: one scalar value per step, the same in every lane
template <class P>
ZL_HD Fp<P> pow_qm3_4(const Fp<P>& a) {
    constexpr int W = SQRT_WINDOW, BITS = P::BITS - 2, NWIN = (BITS + W - 1) / W;
    Fp<P> tab[(1 << W) - 1];  // a^1 .. a^(2^W - 1)
    tab[0] = a;
#pragma unroll
    for (int j = 1; j < (1 << W) - 1; j++) tab[j] = (j & 1) ? zl::sqr(tab[j / 2]) : zl::mul(tab[j - 1], a);
    Fp<P> acc = Fp<P>::one();
#pragma unroll 1
    for (int k = NWIN - 1; k >= 0; k--) {
        const int b = k * W;
        uint32_t d = sqrt_exp_word<P>(b >> 5) >> (b & 31);
        if ((b & 31) + W > 32 && (b >> 5) + 1 < P::N) d |= sqrt_exp_word<P>((b >> 5) + 1) << (32 - (b & 31));
        d &= (1u << W) - 1;
        if (k != NWIN - 1) {
#pragma unroll
            for (int s = 0; s < W; s++) acc = zl::sqr(acc);
        }
        if (d) {  // the exponent is a constant: the same branch in every lane
            Fp<P> t = tab[0];
#pragma unroll
            for (int j = 1; j < (1 << W) - 1; j++) t = select(d == (uint32_t)(j + 1), tab[j], t);
            acc = zl::mul(acc, t);
        }
    }
    return acc;
}
// root = a^((q + 1) / 4) and inv_root = a^((q - 3) / 4) = 1 / root when a is a non-zero square; returns root^2 == a.  When it returns false, root is
// still that power (of no meaning, but a generic value: the decoders carry it on as their dummy y)
template <class P>
ZL_HD bool fq_sqrt_inv(const Fp<P>& a, Fp<P>& root, Fp<P>& inv_root) {
    inv_root = pow_qm3_4(a);
    root = zl::mul(a, inv_root);
    return zl::sqr(root) == a;
}
template <class P>
ZL_HD bool fq_sqrt(const Fp<P>& a, Fp<P>* root) {
    Fp<P> t;
    return fq_sqrt_inv(a, *root, t);
}
// Fq2 = Fq[u] / (u^2 + 1).  Returns root^2 == a; otherwise *root is a value of no meaning, as above.
template <class P>
ZL_HD bool fq2_sqrt(const Fp2<P>& a, Fp2<P>* root) {
    using F = Fp<P>;
    const bool real = a.c1.is_zero();
    F s, ts;
    (void)fq_sqrt_inv(zl::add(zl::sqr(a.c0), zl::sqr(a.c1)), s, ts);  // a is a square only if its norm is one; the last line decides
    // x0^2 is (a0 + s) / 2 or (a0 - s) / 2, whichever is a square; a real a: sqrt(a0), or u sqrt(-a0)
    const F c1 = select(real, a.c0, halve(zl::add(a.c0, s))), c2 = select(real, zl::neg(a.c0), halve(zl::sub(a.c0, s)));
    F r1, t1, r2, t2;
    const bool ok1 = fq_sqrt_inv(c1, r1, t1);
    (void)fq_sqrt_inv(c2, r2, t2);
    const F x0 = select(ok1, r1, r2);
    const F x1 = zl::mul(halve(a.c1), select(ok1, t1, t2));  // a1 / (2 x0); zero for a real a
    const bool swap = real && !ok1;                          // (r2 u)^2 = -r2^2 = a0
    const Fp2<P> r{select(swap, F::zero(), x0), select(swap, x0, x1)};
    *root = r;
    return zl::sqr(r) == a;
}

// canonical integers: a > b  <=>  b - a borrows
template <int N>
ZL_HD bool gt_words(const uint32_t* a, const uint32_t* b) {
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < N; i++) br = (((uint64_t)b[i] - a[i] - br) >> 32) & 1;
    return br != 0;
}
template <class FqP, class FrP, class C1, class C2>
struct Decoder {
    using F = Fp<FqP>;
    using F2 = Fp2<FqP>;
    static constexpr int N = FqP::N, NB = 4 * N;  // words / bytes per Fq element: both moduli leave >= 2 spare bits in their top byte
    static constexpr size_t G1_BYTES = NB, G2_BYTES = 2 * NB;
    static constexpr int G1_WORDS64 = N, G2_WORDS64 = 2 * N;  // u64 words of a decoded point
    // BN254 G1 has cofactor 1: the curve group IS the subgroup of order r (#E(Fq) = r), every point that has a y passes
    static constexpr bool G1_COFACTOR_ONE = std::is_same<FqP, BN254_Fq>::value;

    ZL_HD static F b1() { F r; for (int i = 0; i < N; i++) r.l[i] = C1::b(i); return r; }
    ZL_HD static F2 b2() { F2 r; for (int i = 0; i < N; i++) { r.c0.l[i] = C2::b0(i); r.c1.l[i] = C2::b1(i); } return r; }
    // the x of the generator: what a record without a usable x (malformed, or infinity) computes on, so that it walks the same path as a valid one
    ZL_HD static F dummy_x1() { F r; for (int i = 0; i < N; i++) r.l[i] = C1::gx(i); return r; }
    ZL_HD static F2 dummy_x2() { F2 r; for (int i = 0; i < N; i++) { r.c0.l[i] = C2::gx0(i); r.c1.l[i] = C2::gx1(i); } return r; }

    // r (x, y) == infinity: double-and-add from the top bit of r; bit i is a lookup in the constant words of r by the loop counter, the same in every lane.  The XYZZ formulas are complete
    // (their exceptional cases branch), so a point of small order or off the curve gives a wrong value, not a fault.
    template <class T>
    ZL_HD static bool mul_r_is_inf(const T& x, const T& y) {
        XYZZ<T> acc{x, y, T::one(), T::one()};
#pragma unroll 1
        for (int i = FrP::BITS - 2; i >= 0; i--) {
            zl::dbl_inplace(acc);
            if ((FrP::mod(i >> 5) >> (i & 31)) & 1u) zl::add_mixed(acc, x, y, false);
        }
        return acc.is_inf();
    }
    ZL_HD static bool in_subgroup(const F& x, const F& y) {
        if constexpr (G1_COFACTOR_ONE) return true;  // cofactor 1 (above): no multiplication
        else return mul_r_is_inf(x, y);
    }
    ZL_HD static bool in_subgroup(const F2& x, const F2& y) { return mul_r_is_inf(x, y); }

    // NB little-endian bytes -> words, read bytewise (a record may start at any address).  *top2 = the two flag bits; they are cleared in the words
    ZL_HD static F load_words(const uint8_t* in, uint32_t* top2) {
        F c;
#pragma unroll
        for (int i = 0; i < N; i++)
            c.l[i] = (uint32_t)in[4 * i] | ((uint32_t)in[4 * i + 1] << 8) | ((uint32_t)in[4 * i + 2] << 16) | ((uint32_t)in[4 * i + 3] << 24);
        *top2 = c.l[N - 1] >> 30;
        c.l[N - 1] &= 0x3FFFFFFFu;
        return c;
    }
    ZL_HD static bool lt_q(const F& c) {
        uint32_t q[N];
#pragma unroll
        for (int i = 0; i < N; i++) q[i] = FqP::mod(i);
        return gt_words<N>(q, c.l);
    }
    ZL_HD static void store64(uint64_t* out, const F& c, bool keep) {
#pragma unroll
        for (int i = 0; i < N / 2; i++) out[i] = keep ? ((uint64_t)c.l[2 * i] | ((uint64_t)c.l[2 * i + 1] << 32)) : 0;
    }
    // "y is the larger of {y, -y}" on canonical integers (Fq2: c1 first, then c0, as ark-ff's QuadExtField::cmp)
    ZL_HD static bool larger(const F& yc, const F& nyc) { return gt_words<N>(yc.l, nyc.l); }
    ZL_HD static int status_of(bool malformed, bool is_inf, bool has_y, bool in_group) {
        return malformed ? (int)ZL_EINVAL : is_inf ? (int)ZL_OK : (has_y && in_group) ? (int)ZL_OK : (int)ZL_ENOTCURVE;
    }

    ZL_HD static int decode_g1(const uint8_t* in, uint64_t* xy, uint8_t* inf) {
        uint32_t fl;
        F c = load_words(in, &fl);
        const bool canon = lt_q(c), flag_inf = (fl & 1u) != 0, flag_big = (fl & 2u) != 0;
        const bool malformed = fl == 3u || !canon || (flag_inf && !c.is_zero());
        const F x = select(canon && !flag_inf, zl::to_mont(select(canon, c, F::zero())), dummy_x1());  // (the multiplier takes reduced operands only)
        F y;
        const bool has_y = fq_sqrt(zl::add(zl::mul(zl::sqr(x), x), b1()), &y);
        const bool in_group = in_subgroup(x, y);
        const F yc = zl::from_mont(y), nyc = zl::neg(yc);  // q - yc on the canonical integer (0 stays 0): its limbs are a reduced value like any other
        const F ys = select(larger(yc, nyc) != flag_big, nyc, yc);
        const int st = status_of(malformed, flag_inf, has_y, in_group);
        const bool finite = st == ZL_OK && !flag_inf;
        store64(xy, c, finite);
        store64(xy + N / 2, ys, finite);
        *inf = (st == ZL_OK && flag_inf) ? 1 : 0;
        return st;
    }
    ZL_HD static int decode_g2(const uint8_t* in, uint64_t* xy, uint8_t* inf) {
        uint32_t fl0, fl;
        F c0 = load_words(in, &fl0), c1 = load_words(in + NB, &fl);
        // the host codec reads c0 WITH its top bits (an integer >= 2^(8 NB - 2) > q) and rejects flag bits there explicitly: one condition here
        const bool canon = fl0 == 0 && lt_q(c0) && lt_q(c1), flag_inf = (fl & 1u) != 0, flag_big = (fl & 2u) != 0;
        const bool malformed = fl == 3u || !canon || (flag_inf && !(c0.is_zero() && c1.is_zero()));
        const F2 x = select(canon && !flag_inf, F2{zl::to_mont(select(canon, c0, F::zero())), zl::to_mont(select(canon, c1, F::zero()))}, dummy_x2());
        F2 y;
        const bool has_y = fq2_sqrt(zl::add(zl::mul(zl::sqr(x), x), b2()), &y);
        const bool in_group = in_subgroup(x, y);
        const F2 yc = zl::from_mont(y), nyc = zl::neg(yc);  // component-wise q - c on the canonical integers
        const bool big = yc.c1.is_zero() ? larger(yc.c0, nyc.c0) : larger(yc.c1, nyc.c1);  // c1 == -c1 only for c1 = 0 (q is odd)
        const F2 ys = select(big != flag_big, nyc, yc);
        const int st = status_of(malformed, flag_inf, has_y, in_group);
        const bool finite = st == ZL_OK && !flag_inf;
        store64(xy, c0, finite);
        store64(xy + N / 2, c1, finite);
        store64(xy + N, ys.c0, finite);
        store64(xy + 3 * N / 2, ys.c1, finite);
        *inf = (st == ZL_OK && flag_inf) ? 1 : 0;
        return st;
    }
};

using BlsDecoder = Decoder<BLS12_381_Fq, BLS12_381_Fr, BLS12_381_G1, BLS12_381_G2>;
using BnDecoder = Decoder<BN254_Fq, BN254_Fr, BN254_G1, BN254_G2>;

}  // namespace decode
}  // namespace openzl
