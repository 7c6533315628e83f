// zl_fq12_inv.h -- the inverse of an element of Fq12 = Fq[w]/(w^12 - M6 w^6 + M0_NEG) by a chain of norms, as host-and-device code: the kernel k_pd_fexp
// (zl_pairing_dev.hip) takes its steps from here, one coefficient per lane, and `inverse` below runs the same steps on a whole element on the host (the test
// hook zl_test_fq12_inverse, compared with the oracle's Fq12Ctx.inv).  No elimination, no pivot search, no branch on the data: five Fq12 products and one Fermat
// inversion in Fq, where Engine::inverse (zl_pairing.h) takes twelve.
//
//   1. n6 = f conj6(f), conj6: w -> -w.  n6 is fixed by conj6: its odd coefficients are zero, it is a polynomial in v = w^2.
//   2. sigma: v -> zeta v with zeta a primitive cube root of unity in Fq (the GLV beta of the curve, zl_params.h).  The modulus is a polynomial in v^3, so sigma
//      is an automorphism of order three of Fq[v]; sigma^e multiplies the coefficient of w^(2 j) by zeta^(e j).
//   3. cof = sigma(n6) sigma^2(n6), n2 = n6 cof.  n2 is fixed by sigma: n2 = a0 + a1 u with u = w^6, u^2 = M6 u - M0_NEG; every other coefficient is zero.
//   4. N = n2 (a0 + a1 (M6 - u)) = a0^2 + M6 a0 a1 + M0_NEG a1^2 lies in Fq (M6 - u is the other root of u's polynomial): one Fermat inversion.
//   5. n2^-1 = ((a0 + M6 a1) - a1 u) N^-1,   f^-1 = conj6(f) cof n2^-1.
// N = 0 exactly when f = 0 (Fq12 is a field and every factor of N is a conjugate of f).  The Fermat power of 0 is 0, so a zero input gives the inverse 0 and
// `singular`; nothing else changes.
#pragma once
#include "zl_curve.h"

namespace openzl {
namespace fq12inv {

template <class FqP> struct Glv;
template <> struct Glv<BLS12_381_Fq> { using T = BLS12_381_GLV; };
template <> struct Glv<BN254_Fq> { using T = BN254_GLV; };

// zeta: a primitive cube root of unity in Fq, Montgomery (tests/test_fq12_inverse_chain.py pins zeta^3 = 1, zeta != 1 for both curves)
template <class FqP>
ZL_HD Fp<FqP> zeta() {
    Fp<FqP> z;
    for (int i = 0; i < FqP::N; i++) z.l[i] = Glv<FqP>::T::beta(i);
    return z;
}
// what sigma^e (e = 1, 2) multiplies the coefficient of w^k by: zeta^(e (k / 2) mod 3).  Only even k matter (step 1); an odd k gets the factor of k - 1.
template <class FqP>
ZL_HD Fp<FqP> sigma_factor(int k, int e) {
    const int p = (e * (k >> 1)) % 3;
    const Fp<FqP> z = zeta<FqP>();
    return p == 0 ? Fp<FqP>::one() : p == 1 ? z : zl::sqr(z);
}
// a^(q-2), 0 for a = 0.  The exponent's words come from the modulus' constant table by the loop counter (q's low word is at least 2: no borrow), so the
// power keeps no exponent array in private memory -- zl::inv builds one, which a kernel would hold in scratch.
template <class FqP>
ZL_HD Fp<FqP> fq_inv(const Fp<FqP>& a) {
    static_assert(FqP::mod(0) >= 2u, "q - 2 without a borrow");
    Fp<FqP> acc = Fp<FqP>::one();
    for (int i = 32 * FqP::N - 1; i >= 0; i--) {
        acc = zl::sqr(acc);
        const uint32_t w = FqP::mod(i >> 5) - (i < 32 ? 2u : 0u);
        if ((w >> (i & 31)) & 1) acc = zl::mul(acc, a);
    }
    return acc;
}
// steps 4 and 5: (a0 + a1 u)^-1 = b0 + b1 u; returns N == 0 (then b0 = b1 = 0)
template <class FqP, class PP>
ZL_HD bool quad_inverse(const Fp<FqP>& a0, const Fp<FqP>& a1, Fp<FqP>& b0, Fp<FqP>& b1) {
    const Fp<FqP> m6 = zl::from_u64<FqP>(PP::M6), m0 = zl::from_u64<FqP>(PP::M0_NEG);
    const Fp<FqP> s = zl::add(a0, zl::mul(m6, a1));
    const Fp<FqP> n = zl::add(zl::mul(a0, s), zl::mul(m0, zl::sqr(a1)));
    const Fp<FqP> ni = fq_inv(n);
    b0 = zl::mul(s, ni);
    b1 = zl::neg(zl::mul(a1, ni));
    return n.is_zero();
}

// ---- the chain on a whole element (one thread) ----------------------------------------------------------------------------------------------------
template <class FqP>
struct El {
    Fp<FqP> c[12];
};
template <class FqP, class PP>
ZL_HD El<FqP> mul(const El<FqP>& a, const El<FqP>& b) {
    using F = Fp<FqP>;
    F t[23];
    for (int m = 0; m < 23; m++) t[m] = F::zero();
    for (int i = 0; i < 12; i++)
        for (int j = 0; j < 12; j++) t[i + j] = zl::add(t[i + j], zl::mul(a.c[i], b.c[j]));
    const F m6 = zl::from_u64<FqP>(PP::M6), m0 = zl::from_u64<FqP>(PP::M0_NEG);
    for (int m = 22; m >= 12; m--) {  // w^m = w^(m-12) (M6 w^6 - M0_NEG)
        t[m - 6] = zl::add(t[m - 6], zl::mul(t[m], m6));
        t[m - 12] = zl::sub(t[m - 12], zl::mul(t[m], m0));
    }
    El<FqP> r;
    for (int i = 0; i < 12; i++) r.c[i] = t[i];
    return r;
}
template <class FqP>
ZL_HD El<FqP> conj6(const El<FqP>& a) {
    El<FqP> r;
    for (int k = 0; k < 12; k++) r.c[k] = (k & 1) ? zl::neg(a.c[k]) : a.c[k];
    return r;
}
template <class FqP>
ZL_HD El<FqP> sigma(const El<FqP>& a, int e) {
    El<FqP> r;
    for (int k = 0; k < 12; k++) r.c[k] = zl::mul(a.c[k], sigma_factor<FqP>(k, e));
    return r;
}
template <class FqP, class PP>
ZL_HD El<FqP> inverse(const El<FqP>& f, bool* singular) {
    const El<FqP> c = conj6(f);
    const El<FqP> n6 = mul<FqP, PP>(f, c);
    const El<FqP> cof = mul<FqP, PP>(sigma(n6, 1), sigma(n6, 2));
    const El<FqP> n2 = mul<FqP, PP>(n6, cof);
    El<FqP> ni;
    for (int k = 0; k < 12; k++) ni.c[k] = Fp<FqP>::zero();
    *singular = quad_inverse<FqP, PP>(n2.c[0], n2.c[6], ni.c[0], ni.c[6]);
    return mul<FqP, PP>(mul<FqP, PP>(c, cof), ni);
}

}  // namespace fq12inv
}  // namespace openzl
