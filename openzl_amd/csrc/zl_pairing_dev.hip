// zl_pairing_dev.hip -- Miller loops of many pairings on the device (the product side of PairingEngine::product_of_pairings, which the plugin's
// PairingEngineExt helpers and Groth16 verification call: the reference plugin's plugins/arkworks/src/pairing.rs:47-90, groth16.rs:459-466).
// Compiled once per curve (ZL_PAIR_CURVE = 1 BLS12-381, 2 BN254); the host final exponentiation (zl_pairing.h Engine::final_exp) turns the
// product into the pairing (zl_verify.hip: zl_pairing_product, zl_groth16_verify_batch).
//
// Same Fq12 as zl_pairing.h: Fq[w]/(w^12 - M6 w^6 + M0_NEG), 12 Fq coefficients, the same loop schedule (LOOP_BITS / loop_bit, BN_TAIL lines) and the same
// line placement (put_fq2; TWIST_DIV: BLS12-381 M-type twist).  Differences to the host loop, all annihilated by the final exponentiation (q^12 - 1)/r:
//   - G2 walks in homogeneous projective coordinates (X : Y : Z) on the twist, no inversion.  The tangent line at R is scaled by 2 Y Z^2 (an Fq2 factor),
//     the line through R and an affine Q by lambda = xQ Z - X (Fq2):
//         tangent:  c0 = 2 Y^2 Z - 3 X^3,     cx = 3 X^2 Z,   cy = -2 Y Z^2
//         chord:    c0 = yQ lambda - theta xQ, cx = theta,     cy = -lambda        (theta = yQ Z - Y)
//     and the line is c0 + cx xP + cy yP placed like zl_pairing.h's  (y1' - m' x1') + (m' xP) + (-yP)  terms.  Fq2* has order dividing q^6 - 1.
//   - P may be given in XYZZ coordinates (x = X/ZZ, y = Y/ZZZ: the batch verifier's rho_i A_i): c0 ZZ ZZZ + cx X ZZZ + cy Y ZZ is the line times the Fq factor ZZ ZZZ.
// The Miller values therefore differ from the host's before the final exponentiation; after it they are equal (tests/test_gpu_pairing_product.py).
//
// Kernels:
//   k_pd_prep   one lane per pair: canonical inputs -> Montgomery, the optional 128-bit scalar multiplication of P (double-and-add in XYZZ), infinity flags.
//   k_pd_lines  one lane per pair walks R on the twist and writes its NLINES line records (six Fq coefficients each, already multiplied by xP / yP) to HBM,
//               laid out [step][pair][6][N words] so that a wave writes one contiguous block per step.
//   k_pd_acc    16-lane groups (12 active lanes, lane k owns coefficient w^k of the accumulator f; operands exchanged through LDS): per step
//               f <- f^2 prod_{pairs of the group} l_i -- one shared squaring per group and step.  Pair p belongs to group p % ngroups.
//   k_pd_prod   product of the group accumulators, 16 at a time per group of lanes, until one is left.
//   k_pd_fexp   the final exponentiation (q^12 - 1)/r of one Fq12 value per 16-lane group, Engine::final_exp's schedule: g = conj6(f) / f with the inverse by the
//               norm chain of zl_fq12_inv.h, then g^((q^6 + 1)/r) in 4-bit fixed windows over PP::final_exp().  The 15 window powers of a group live in HBM
//               (ZL_SLOT_PAIR_FEXP); squarings use the symmetry of Engine::sqr (7 products per lane instead of 12).
// Plain Fp<Fq> (32-bit limbs, fully reduced): no lazily reduced formulas, so nothing new for zl_bounds.h.  Every loop bound is a compile-time constant or a
// launch argument: off-curve / non-subgroup inputs give a wrong value (or a zero product, which the host reports as ZL_ENOTCURVE), never a different path.
#include <string.h>
#include <algorithm>
#include <vector>
#include "zl_ctx.h"
#include "zl_fq12_inv.h"
#include "zl_pairing.h"
#include "zl_pairing_dev.h"

#if ZL_PAIR_CURVE == 1
#define ZL_PD_FQ BLS12_381_Fq
#define ZL_PD_PP BLS12_381_Pairing
#define ZL_PD_SUFFIX(x) x##_bls
#else
#define ZL_PD_FQ BN254_Fq
#define ZL_PD_PP BN254_Pairing
#define ZL_PD_SUFFIX(x) x##_bn
#endif

namespace {
using FqP = ZL_PD_FQ;
using PP = ZL_PD_PP;
using F = Fp<FqP>;
using F2 = Fp2<FqP>;
constexpr int NW = FqP::N;  // u32 words per Fq
constexpr int nadd() {
    int c = 0;
    for (int i = PP::LOOP_BITS - 2; i >= 0; i--) c += PP::loop_bit(i) ? 1 : 0;
    return c;
}
constexpr int NLINES = PP::LOOP_BITS - 1 + nadd() + (PP::BN_TAIL ? 2 : 0);  // 68 (BLS12-381), 64 + 21 + 2 = 87 (BN254)
// the three Fq2 terms of a line and where put_fq2 places them (coefficients k and k + 6)
constexpr int K0 = PP::TWIST_DIV ? 0 : 3, KX = PP::TWIST_DIV ? 2 : 1, KY = PP::TWIST_DIV ? 3 : 0;
__host__ __device__ constexpr int line_pos(int m) { return (m & 1 ? 6 : 0) + (m < 2 ? K0 : m < 4 ? KX : KY); }
constexpr int M_ONE = K0 == 0 ? 0 : KX == 0 ? 2 : 4;  // the record slot of coefficient w^0 (where a line equal to 1 puts its 1)

struct Consts {
    F sh, m6, nm0, m6sq_m0, nm6m0;  // ISHIFT, M6, -M0_NEG, M6^2 - M0_NEG, -M6 M0_NEG (Montgomery)
    F2 g2, g3;                      // Frobenius constants of the BN tail (zl_pairing.h make_frob_consts)
};

__device__ __forceinline__ F2 f2s(const F2& a, const F& s) { return F2{zl::mul(a.c0, s), zl::mul(a.c1, s)}; }
__device__ __forceinline__ F2 conj(const F2& a) { return F2{a.c0, zl::neg(a.c1)}; }

// one line record: c0 zP + cx xP + cy yP placed by put_fq2; `one` replaces it by 1 (a pair with a point at infinity, or padding)
__device__ __forceinline__ void emit(F* rec, const F2& c0, const F2& cx, const F2& cy, const F& xP, const F& yP, const F& zP, bool one, const Consts& K) {
    const F2 a = f2s(c0, zP), b = f2s(cx, xP), c = f2s(cy, yP);
    F v[6] = {zl::sub(a.c0, zl::mul(K.sh, a.c1)), a.c1, zl::sub(b.c0, zl::mul(K.sh, b.c1)), b.c1, zl::sub(c.c0, zl::mul(K.sh, c.c1)), c.c1};
#pragma unroll
    for (int m = 0; m < 6; m++) rec[m] = one ? (m == M_ONE ? F::one() : F::zero()) : v[m];
}
// R <- 2R, line at the tangent (scaled by 2 Y Z^2)
__device__ __forceinline__ void dbl_step(F2& X, F2& Y, F2& Z, F2& c0, F2& cx, F2& cy) {
    const F2 xx = zl::sqr(X), yy = zl::sqr(Y);
    const F2 w = zl::add(zl::dbl(xx), xx);            // 3 X^2
    const F2 s = zl::mul(Y, Z);                       // S = Y Z
    c0 = zl::sub(zl::dbl(zl::mul(yy, Z)), zl::mul(w, X));
    cx = zl::mul(w, Z);
    cy = zl::neg(zl::dbl(zl::mul(s, Z)));
    const F2 b = zl::mul(zl::mul(X, Y), s);           // B = X Y S
    const F2 b4 = zl::dbl(zl::dbl(b));
    const F2 h = zl::sub(zl::sqr(w), zl::dbl(b4));    // H = W^2 - 8B
    const F2 ss = zl::sqr(s);
    X = zl::dbl(zl::mul(h, s));
    Y = zl::sub(zl::mul(w, zl::sub(b4, h)), zl::dbl(zl::dbl(zl::dbl(zl::mul(yy, ss)))));
    Z = zl::dbl(zl::dbl(zl::dbl(zl::mul(s, ss))));
}
// R <- R + Q (Q affine), line through R and Q (scaled by lambda = xQ Z - X)
__device__ __forceinline__ void add_step(F2& X, F2& Y, F2& Z, const F2& xq, const F2& yq, F2& c0, F2& cx, F2& cy) {
    const F2 th = zl::sub(zl::mul(yq, Z), Y), la = zl::sub(zl::mul(xq, Z), X);
    c0 = zl::sub(zl::mul(yq, la), zl::mul(th, xq));
    cx = th;
    cy = zl::neg(la);
    const F2 uu = zl::sqr(th), vv = zl::sqr(la), vvv = zl::mul(la, vv), rr = zl::mul(vv, X);
    const F2 a = zl::sub(zl::sub(zl::mul(uu, Z), vvv), zl::dbl(rr));
    X = zl::mul(la, a);
    Y = zl::sub(zl::mul(th, zl::sub(rr, a)), zl::mul(vvv, Y));
    Z = zl::mul(vvv, Z);
}

__device__ __forceinline__ F load_canon64(const uint64_t* w) {  // canonical u64 words -> Montgomery
    F c;
#pragma unroll
    for (int i = 0; i < NW / 2; i++) {
        c.l[2 * i] = (uint32_t)w[i];
        c.l[2 * i + 1] = (uint32_t)(w[i] >> 32);
    }
    return zl::to_mont(c);
}

// inputs -> Montgomery records: pm[p] = (xP', yP', zP) with zP = 0 for a pair that contributes 1 (a point at infinity, padding), qm[p] = (xQ, yQ)
__global__ __launch_bounds__(64) void k_pd_prep(const uint64_t* __restrict__ ps, const uint64_t* __restrict__ qs, const uint32_t* __restrict__ sc, size_t n,
                                                size_t npad, F* __restrict__ pm, F2* __restrict__ qm) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npad) return;
    const size_t pl = p < n ? p : 0;  // padding lanes read pair 0 and are marked as ones
    F xP = load_canon64(ps + pl * NW), yP = load_canon64(ps + pl * NW + NW / 2), zP = F::one();
    bool one = p >= n || (xP.is_zero() && yP.is_zero());
    if (sc) {  // P <- k P for a 128-bit k (XYZZ, the line absorbs the Fq factor zz zzz)
        XYZZ<F> acc = XYZZ<F>::inf();
        for (int i = 127; i >= 0; i--) {
            zl::dbl_inplace(acc);
            if ((sc[4 * pl + (i >> 5)] >> (i & 31)) & 1) zl::add_mixed(acc, xP, yP, false);
        }
        one = one || acc.is_inf();
        xP = zl::mul(acc.x, acc.zzz);
        yP = zl::mul(acc.y, acc.zz);
        zP = zl::mul(acc.zz, acc.zzz);
    }
    const uint64_t* q = qs + pl * 2 * NW;
    const F2 xq{load_canon64(q), load_canon64(q + NW / 2)}, yq{load_canon64(q + NW), load_canon64(q + 3 * NW / 2)};
    one = one || (xq.is_zero() && yq.is_zero());
    pm[3 * p] = xP;
    pm[3 * p + 1] = yP;
    pm[3 * p + 2] = one ? F::zero() : zP;
    qm[2 * p] = xq;
    qm[2 * p + 1] = yq;
}

__global__ __launch_bounds__(64) void k_pd_lines(const F* __restrict__ pm, const F2* __restrict__ qm, size_t npad, Consts K, F* __restrict__ lines) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npad) return;
    const F xP = pm[3 * p], yP = pm[3 * p + 1], zP = pm[3 * p + 2];
    const bool one = zP.is_zero();
    // Q is read again at every addition step instead of being held through the doublings (register budget)
    F2 X = qm[2 * p], Y = qm[2 * p + 1], Z = F2::one(), c0, cx, cy;
    F* rec = lines + p * 6;
    const size_t step = npad * 6;
    for (int i = PP::LOOP_BITS - 2; i >= 0; i--) {
        dbl_step(X, Y, Z, c0, cx, cy);
        emit(rec, c0, cx, cy, xP, yP, zP, one, K);
        rec += step;
        if (PP::loop_bit(i)) {
            add_step(X, Y, Z, qm[2 * p], qm[2 * p + 1], c0, cx, cy);
            emit(rec, c0, cx, cy, xP, yP, zP, one, K);
            rec += step;
        }
    }
    if (PP::BN_TAIL) {
        const F2 x1 = zl::mul(conj(qm[2 * p]), K.g2), y1 = zl::mul(conj(qm[2 * p + 1]), K.g3);
        const F2 x2 = zl::mul(conj(x1), K.g2), y2 = zl::neg(zl::mul(conj(y1), K.g3));
        add_step(X, Y, Z, x1, y1, c0, cx, cy);
        emit(rec, c0, cx, cy, xP, yP, zP, one, K);
        rec += step;
        add_step(X, Y, Z, x2, y2, c0, cx, cy);
        emit(rec, c0, cx, cy, xP, yP, zP, one, K);
    }
}

// ---- Fq12 products on a group of 16 lanes (lane k < 12 owns coefficient w^k) ---------------------------------------------------------------
// t[m] = sum_{i+j=m} a_i b_j, lane k computes t[k] (i <= k) and t[k+12] (i > k): 12 products per lane for a full product, 6 for a line (whose six
// non-zero coefficients each meet exactly one a_i per lane).  Then w^m = w^(m-12) (M6 w^6 - M0_NEG) folds t[12..22] back:
//   c_k = t[k] + [k >= 6] M6 t[k+6] + (k <= 5 ? -M0 : M6^2 - M0) t[k+12] + [k <= 4] (-M6 M0) t[k+18]      (t[23] = 0 stands in for absent terms)
__device__ __forceinline__ F fold(const F* t, int k, const Consts& K) {
    F c = zl::add(t[k], zl::mul(t[k + 12], k <= 5 ? K.nm0 : K.m6sq_m0));
    c = zl::add(c, zl::mul(t[k >= 6 ? k + 6 : 23], K.m6));
    return zl::add(c, zl::mul(t[k <= 4 ? k + 18 : 23], K.nm6m0));
}
// fk <- (sum_i a_i w^i)(sum_j b_j w^j) with a, b in LDS; three barriers (the caller's LDS writes must precede the call)
__device__ __forceinline__ void mul_full(F& fk, const F* a, const F* b, F* t, int k, bool act, const Consts& K) {
    __syncthreads();
    if (act) {
        F lo = F::zero(), hi = F::zero();
#pragma unroll 1
        for (int i = 0; i < 12; i++) {
            const int j = k - i;
            const F pr = zl::mul(a[i], b[j >= 0 ? j : j + 12]);
            if (j >= 0) lo = zl::add(lo, pr);
            else hi = zl::add(hi, pr);
        }
        t[k] = lo;
        t[k + 12] = hi;
    }
    __syncthreads();
    if (act) fk = fold(t, k, K);
    __syncthreads();
}
// fk <- f * line (six coefficients at line_pos(m), read from HBM)
__device__ __forceinline__ void mul_line(F& fk, F* a, const F* __restrict__ rec, F* t, int k, bool act, const Consts& K) {
    if (act) a[k] = fk;
    __syncthreads();
    if (act) {
        F lo = F::zero(), hi = F::zero();
#pragma unroll
        for (int m = 0; m < 6; m++) {
            const int j = line_pos(m), i = k - j;
            const F pr = zl::mul(a[i >= 0 ? i : i + 12], rec[m]);
            if (i >= 0) lo = zl::add(lo, pr);
            else hi = zl::add(hi, pr);
        }
        t[k] = lo;
        t[k + 12] = hi;
    }
    __syncthreads();
    if (act) fk = fold(t, k, K);
    __syncthreads();
}

__global__ __launch_bounds__(64) void k_pd_acc(const F* __restrict__ lines, size_t npad, uint32_t ngroups, uint32_t G, Consts K, F* __restrict__ acc) {
    __shared__ F sa[4][12];
    __shared__ F st[4][24];
    const int grp = threadIdx.x >> 4, k = threadIdx.x & 15;
    const uint32_t g = blockIdx.x * 4 + grp;
    const bool act = k < 12 && g < ngroups;
    F* a = sa[grp];
    F* t = st[grp];
    if (act && k == 11) t[23] = F::zero();
    F fk = k == 0 ? F::one() : F::zero();
    const size_t step = npad * 6;
    const F* rec = lines + (size_t)(act ? g : 0) * 6;
    for (int i = PP::LOOP_BITS - 2; i >= 0; i--) {
        if (act) a[k] = fk;
        mul_full(fk, a, a, t, k, act, K);
#pragma unroll 1
        for (uint32_t j = 0; j < G; j++) mul_line(fk, a, rec + (size_t)j * ngroups * 6, t, k, act, K);
        rec += step;
        if (PP::loop_bit(i)) {
#pragma unroll 1
            for (uint32_t j = 0; j < G; j++) mul_line(fk, a, rec + (size_t)j * ngroups * 6, t, k, act, K);
            rec += step;
        }
    }
    if (PP::BN_TAIL) {
#pragma unroll 1
        for (int e = 0; e < 2; e++) {
#pragma unroll 1
            for (uint32_t j = 0; j < G; j++) mul_line(fk, a, rec + (size_t)j * ngroups * 6, t, k, act, K);
            rec += step;
        }
    }
    if (act) acc[(size_t)g * 12 + k] = fk;
}

// out[g] = prod of in[g * per .. g * per + per) (entries >= cnt count as 1)
__global__ __launch_bounds__(64) void k_pd_prod(const F* __restrict__ in, uint32_t cnt, uint32_t per, uint32_t nout, Consts K, F* __restrict__ out) {
    __shared__ F sa[4][12];
    __shared__ F sb[4][12];
    __shared__ F st[4][24];
    const int grp = threadIdx.x >> 4, k = threadIdx.x & 15;
    const uint32_t g = blockIdx.x * 4 + grp;
    const bool act = k < 12 && g < nout;
    F* a = sa[grp];
    F* b = sb[grp];
    F* t = st[grp];
    if (act && k == 11) t[23] = F::zero();
    F fk = k == 0 ? F::one() : F::zero();
#pragma unroll 1
    for (uint32_t e = 0; e < per; e++) {
        const size_t idx = (size_t)g * per + e;
        if (act) {
            a[k] = fk;
            b[k] = idx < cnt ? in[idx * 12 + k] : (k == 0 ? F::one() : F::zero());
        }
        mul_full(fk, a, b, t, k, act, K);
    }
    if (act) out[(size_t)g * 12 + k] = fk;
}

// fk <- f^2 with f's coefficients in the lanes' fk: t[m] = sum_{i<=j, i+j=m} (i < j ? 2 : 1) a_i a_j.  Lane k has k/2 + 1 such pairs for t[k] and 6 - ceil(k/2) for
// t[k+12]: seven steps for an even k, six for an odd one (whose seventh step is empty), where mul_full takes twelve.
__device__ __forceinline__ void sqr_full(F& fk, F* a, F* t, int k, bool act, const Consts& K) {
    if (act) a[k] = fk;
    __syncthreads();
    if (act) {
        F lo = F::zero(), hi = F::zero();
        const int h = k >> 1;
#pragma unroll 1
        for (int s = 0; s < 7; s++) {
            const bool low = s <= h;
            const int i = low ? s : k + s - h, j = (low ? k : k + 12) - i;
            if (i <= j) {
                F pr = zl::mul(a[i], a[j]);
                if (i != j) pr = zl::dbl(pr);
                if (low) lo = zl::add(lo, pr);
                else hi = zl::add(hi, pr);
            }
        }
        t[k] = lo;
        t[k + 12] = hi;
    }
    __syncthreads();
    if (act) fk = fold(t, k, K);
    __syncthreads();
}

constexpr int FEXP_TAB = 15;  // window powers g^1 .. g^15 of a value (g^0 = 1 is never multiplied in)
// out[g] = in[g]^((q^12 - 1)/r), Montgomery in and out (out may be in); singular[g] = (in[g] == 0), whose result is 0.  ew: the words of PP::final_exp().
// The exponent is the same for every group, so the branches on its nibbles are uniform over the launch; nothing depends on the values.
__global__ __launch_bounds__(64) void k_pd_fexp(const F* in, uint32_t count, Consts K, const uint32_t* __restrict__ ew, F* tab, F* out, uint8_t* __restrict__ singular) {
    __shared__ F sa[4][12];
    __shared__ F sb[4][12];
    __shared__ F st[4][24];
    const int grp = threadIdx.x >> 4, k = threadIdx.x & 15;
    const uint32_t g = blockIdx.x * 4 + grp;
    const bool act = k < 12 && g < count;
    F* a = sa[grp];
    F* b = sb[grp];
    F* t = st[grp];
    if (act && k == 11) t[23] = F::zero();
    F* T = tab + (size_t)(act ? g : 0) * FEXP_TAB * 12 + (act ? k : 0);  // this lane's coefficient of g^e at T[(e - 1) * 12]
    const F fk = act ? in[(size_t)g * 12 + k] : F::zero();
    const F ck = (k & 1) ? zl::neg(fk) : fk;  // conj6(f)
    // f^-1 (zl_fq12_inv.h): n6 = f conj6(f)
    F n6 = F::zero(), cof = F::zero(), x = F::zero();
    if (act) {
        a[k] = fk;
        b[k] = ck;
    }
    mul_full(n6, a, b, t, k, act, K);
    // cof = sigma(n6) sigma^2(n6)
    if (act) {
        a[k] = zl::mul(n6, openzl::fq12inv::sigma_factor<FqP>(k, 1));
        b[k] = zl::mul(n6, openzl::fq12inv::sigma_factor<FqP>(k, 2));
    }
    mul_full(cof, a, b, t, k, act, K);
    // n2 = n6 cof = a0 + a1 w^6
    if (act) {
        a[k] = n6;
        b[k] = cof;
    }
    mul_full(x, a, b, t, k, act, K);
    // n2^-1 = b0 + b1 w^6 on lane 0 of the group (one Fermat inversion in Fq), left in b
    if (act) {
        a[k] = x;
        if (k != 0 && k != 6) b[k] = F::zero();
    }
    __syncthreads();
    if (act && k == 0) {
        F b0, b1;
        const bool z = openzl::fq12inv::quad_inverse<FqP, PP>(a[0], a[6], b0, b1);
        b[0] = b0;
        b[6] = b1;
        singular[g] = z ? 1 : 0;
    }
    __syncthreads();
    // g = conj6(f) f^-1 = conj6(f)^2 cof n2^-1
    if (act) a[k] = cof;
    mul_full(x, a, b, t, k, act, K);
    if (act) {
        a[k] = x;
        b[k] = ck;
    }
    mul_full(x, a, b, t, k, act, K);
    if (act) {
        a[k] = x;
        b[k] = ck;
    }
    mul_full(x, a, b, t, k, act, K);
    // the window powers: g^e = g^(e-1) g for an odd e, (g^(e/2))^2 for an even one (each lane reads back only what it wrote itself)
    const F gk = x;
    if (act) T[0] = x;
#pragma unroll 1
    for (int e = 2; e <= FEXP_TAB; e++) {
        if (e & 1) {
            if (act) {
                a[k] = x;
                b[k] = gk;
            }
            mul_full(x, a, b, t, k, act, K);
        } else {
            if (act) x = T[(size_t)((e >> 1) - 1) * 12];
            sqr_full(x, a, t, k, act, K);
        }
        if (act) T[(size_t)(e - 1) * 12] = x;
    }
    F acc = k == 0 ? F::one() : F::zero();
    bool started = false;
#pragma unroll 1
    for (int i = PP::FINAL_EXP_WORDS * 8 - 1; i >= 0; i--) {
        const uint32_t nib = (ew[i >> 3] >> (4 * (i & 7))) & 15u;
        if (started) {
#pragma unroll 1
            for (int s = 0; s < 4; s++) sqr_full(acc, a, t, k, act, K);
        }
        if (nib) {
            if (started) {
                if (act) {
                    a[k] = acc;
                    b[k] = T[(size_t)(nib - 1) * 12];
                }
                mul_full(acc, a, b, t, k, act, K);
            } else {
                if (act) acc = T[(size_t)(nib - 1) * 12];
                started = true;
            }
        }
    }
    if (act) out[(size_t)g * 12 + k] = acc;
}

Consts make_consts() {
    using Eng = openzl::pairing::Engine<FqP, PP>;
    Consts K;
    K.sh = zl::from_u64<FqP>(PP::ISHIFT);
    K.m6 = zl::from_u64<FqP>(PP::M6);
    K.nm0 = zl::neg(zl::from_u64<FqP>(PP::M0_NEG));
    K.m6sq_m0 = zl::from_u64<FqP>((uint64_t)PP::M6 * PP::M6 - PP::M0_NEG);
    K.nm6m0 = zl::neg(zl::from_u64<FqP>((uint64_t)PP::M6 * PP::M0_NEG));
    if (PP::BN_TAIL) {
        const auto fc = Eng::make_frob_consts();
        K.g2 = fc.g2;
        K.g3 = fc.g3;
    } else {
        K.g2 = K.g3 = F2::one();
    }
    return K;
}

// one launch set: pairs [0, n) in ngroups groups -> `reduce ? 1 : ngroups` Fq12 values in out (Montgomery words).  With d_res the values stay on the device:
// *d_res points at them (inside ZL_SLOT_PAIR_ACC), nothing is copied and the stream is not drained -- the caller goes on with them on ctx->stream.
int run(zl_ctx* ctx, const uint64_t* ps, const uint64_t* qs, const uint32_t* sc, size_t n, size_t ngroups, bool reduce, uint32_t* out, const F** d_res = nullptr) {
    if (!ctx || (!out && !d_res) || n == 0 || ngroups == 0 || ngroups > n || n > openzl::pairing_dev::MAX_PAIRS) return ZL_EINVAL;
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    static const Consts K = make_consts();
    const size_t G = (n + ngroups - 1) / ngroups, npad = G * ngroups;
    const size_t pb = n * NW * 8, qb = 2 * pb, sb = sc ? n * 16 : 0;  // bytes of ps (n x 2 Fq of NW u32), qs (n x 4 Fq), scalars
    const size_t in_bytes = (pb + qb + sb + 255) & ~(size_t)255;
    void *d_in = nullptr, *d_lines = nullptr, *d_acc = nullptr, *d_prep = nullptr;
    int rc = zl_scratch_get(ctx, ZL_SLOT_PAIR_IN, in_bytes, &d_in);
    if (!rc) rc = zl_scratch_get(ctx, ZL_SLOT_PAIR_PREP, npad * 7 * sizeof(F), &d_prep);
    if (!rc) rc = zl_scratch_get(ctx, ZL_SLOT_PAIR_LINES, (size_t)NLINES * npad * 6 * sizeof(F), &d_lines);
    const size_t nred = (ngroups + 15) / 16;
    if (!rc) rc = zl_scratch_get(ctx, ZL_SLOT_PAIR_ACC, (ngroups + nred + 1) * 12 * sizeof(F), &d_acc);
    if (rc) return rc;
    unsigned char* din = static_cast<unsigned char*>(d_in);
    ZL_HIP(ctx, hipMemcpyAsync(din, ps, pb, hipMemcpyHostToDevice, ctx->stream));
    ZL_HIP(ctx, hipMemcpyAsync(din + pb, qs, qb, hipMemcpyHostToDevice, ctx->stream));
    if (sc) ZL_HIP(ctx, hipMemcpyAsync(din + pb + qb, sc, sb, hipMemcpyHostToDevice, ctx->stream));
    F* lines = static_cast<F*>(d_lines);
    F* acc = static_cast<F*>(d_acc);
    F* pm = static_cast<F*>(d_prep);
    F2* qm = reinterpret_cast<F2*>(pm + 3 * npad);
    hipLaunchKernelGGL(k_pd_prep, dim3((unsigned)((npad + 63) / 64)), dim3(64), 0, ctx->stream, reinterpret_cast<const uint64_t*>(din),
                       reinterpret_cast<const uint64_t*>(din + pb), sc ? reinterpret_cast<const uint32_t*>(din + pb + qb) : nullptr, n, npad, pm, qm);
    ZL_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_pd_lines, dim3((unsigned)((npad + 63) / 64)), dim3(64), 0, ctx->stream, pm, qm, npad, K, lines);
    ZL_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_pd_acc, dim3((unsigned)((ngroups + 3) / 4)), dim3(64), 0, ctx->stream, lines, npad, (uint32_t)ngroups, (uint32_t)G, K, acc);
    ZL_HIP(ctx, hipGetLastError());
    const F* res = acc;
    size_t cnt = ngroups;
    if (reduce) {
        F* bufs[2] = {acc + ngroups * 12, acc};  // the levels ping-pong between the space behind the accumulators (nred entries) and their own
        int side = 0;
        while (cnt > 1) {
            const size_t nout = (cnt + 15) / 16;
            hipLaunchKernelGGL(k_pd_prod, dim3((unsigned)((nout + 3) / 4)), dim3(64), 0, ctx->stream, res, (uint32_t)cnt, 16u, (uint32_t)nout, K, bufs[side]);
            ZL_HIP(ctx, hipGetLastError());
            res = bufs[side];
            side ^= 1;
            cnt = nout;
        }
    }
    if (d_res) {
        *d_res = res;
        return ZL_OK;
    }
    ZL_HIP(ctx, hipMemcpyAsync(out, res, cnt * 12 * sizeof(F), hipMemcpyDeviceToHost, ctx->stream));
    ZL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZL_OK;
}

// count final exponentiations, ZL_TUNE_FEXP_CHUNK values per launch: d_in (device, Montgomery; a groups launch of run()) or, when it is null, h_in (host)
// -> out (host, Montgomery), singular (host, optional).  ZL_SLOT_PAIR_FEXP: exponent words | count values | count flags | the window powers of one launch.
int fexp(zl_ctx* ctx, const F* d_in, const uint32_t* h_in, size_t count, uint32_t* out, uint8_t* singular) {
    if (!ctx || !out || (!d_in && !h_in)) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    static const Consts K = make_consts();
    const int tune = zl_tune("ZL_TUNE_FEXP_CHUNK", (int)openzl::pairing_dev::FEXP_CHUNK);
    const size_t chunk = std::min(count, (size_t)(tune < 1 ? 1 : tune));
    auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t ew_bytes = pad(PP::FINAL_EXP_WORDS * 4), val_bytes = pad(count * 12 * sizeof(F)), sing_bytes = pad(count);
    void* d = nullptr;
    const int rc = zl_scratch_get(ctx, ZL_SLOT_PAIR_FEXP, ew_bytes + val_bytes + sing_bytes + chunk * FEXP_TAB * 12 * sizeof(F), &d);
    if (rc) return rc;
    unsigned char* base = static_cast<unsigned char*>(d);
    uint32_t* ew = reinterpret_cast<uint32_t*>(base);
    F* vals = reinterpret_cast<F*>(base + ew_bytes);
    uint8_t* sing = base + ew_bytes + val_bytes;
    F* tab = reinterpret_cast<F*>(base + ew_bytes + val_bytes + sing_bytes);
    ZL_HIP(ctx, hipMemcpyAsync(ew, PP::final_exp(), PP::FINAL_EXP_WORDS * 4, hipMemcpyHostToDevice, ctx->stream));
    if (!d_in) {
        ZL_HIP(ctx, hipMemcpyAsync(vals, h_in, count * 12 * sizeof(F), hipMemcpyHostToDevice, ctx->stream));
        d_in = vals;  // in place: a lane reads its coefficient before anything is written
    }
    for (size_t first = 0; first < count; first += chunk) {
        const size_t m = std::min(chunk, count - first);
        hipLaunchKernelGGL(k_pd_fexp, dim3((unsigned)((m + 3) / 4)), dim3(64), 0, ctx->stream, d_in + first * 12, (uint32_t)m, K, ew, tab, vals + first * 12, sing + first);
        ZL_HIP(ctx, hipGetLastError());
    }
    ZL_HIP(ctx, hipMemcpyAsync(out, vals, count * 12 * sizeof(F), hipMemcpyDeviceToHost, ctx->stream));
    if (singular) ZL_HIP(ctx, hipMemcpyAsync(singular, sing, count, hipMemcpyDeviceToHost, ctx->stream));
    ZL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZL_OK;
}
}  // namespace

namespace openzl {
namespace pairing_dev {
int ZL_PD_SUFFIX(miller_groups)(zl_ctx* ctx, const uint64_t* ps, const uint64_t* qs, const uint32_t* sc, size_t n, size_t ngroups, uint32_t* out) {
    return run(ctx, ps, qs, sc, n, ngroups, false, out);
}
int ZL_PD_SUFFIX(miller_product)(zl_ctx* ctx, const uint64_t* ps, const uint64_t* qs, const uint32_t* sc, size_t n, uint32_t* out) {
    using Eng = openzl::pairing::Engine<FqP, PP>;
    if (!ctx || !out || (n && (!ps || !qs))) return ZL_EINVAL;
    typename Eng::Fq12 f = Eng::one();
    // groups per launch: about 32 per CU (8 waves of 4 groups): below that a pair gets a group of its own, above it pairs share squarings.
    // ZL_TUNE_PAIR_GROUPS (>= 1) and ZL_TUNE_PAIR_SET (clamped to [1, MAX_PAIRS]) lower the two numbers so that tests reach shared groups, padding
    // lanes and several launch sets at tens of pairs; run() still checks against MAX_PAIRS and the scratch sizing is unchanged.
    const int tune_groups = zl_tune("ZL_TUNE_PAIR_GROUPS", 0);
    const size_t target = tune_groups >= 1 ? (size_t)tune_groups : (size_t)(ctx->cu_count > 0 ? ctx->cu_count : 256) * 32;
    const size_t set = pair_set(zl_tune("ZL_TUNE_PAIR_SET", (int)MAX_PAIRS));
    for (size_t first = 0; first < n; first += set) {
        const size_t m = n - first < set ? n - first : set;
        const size_t G = (m + target - 1) / target, ng = (m + G - 1) / G;
        typename Eng::Fq12 part;
        const int rc = run(ctx, ps + first * NW, qs + first * 2 * NW, sc ? sc + 4 * first : nullptr, m, ng, true, reinterpret_cast<uint32_t*>(part.c));
        if (rc) return rc;
        f = Eng::mul(f, part);
    }
    memcpy(out, f.c, sizeof f.c);
    return ZL_OK;
}
int ZL_PD_SUFFIX(final_exp)(zl_ctx* ctx, const uint32_t* in, size_t count, uint32_t* out, uint8_t* singular) {
    if (count && !in) return ZL_EINVAL;
    return fexp(ctx, nullptr, in, count, out, singular);
}
int ZL_PD_SUFFIX(pairing_groups)(zl_ctx* ctx, const uint64_t* ps, const uint64_t* qs, const uint32_t* sc, size_t n, size_t ngroups, uint32_t* out, uint8_t* singular) {
    const F* d_f = nullptr;
    const int rc = run(ctx, ps, qs, sc, n, ngroups, false, nullptr, &d_f);
    return rc ? rc : fexp(ctx, d_f, nullptr, ngroups, out, singular);
}
}  // namespace pairing_dev
}  // namespace openzl
