// zl_msm_cover_plan.h -- the exact-cover window plan of a split G1 MSM: the two 127-bit half-scalars of k = k1 + k2 lambda are recoded into windows whose
// widths sum to exactly 128 bits (22, 21, 21, 21, 21, 22 at 2^24 points), so that every half has six signed digits -- twelve entries per point where thirteen
// plain 20-bit windows need thirteen -- and no window is narrower than the others.  The device keeps UNIFORM bucket sets of 2^set_log buckets: a window of width
// w owns 2^(w - 1 - set_log) consecutive sets (the top window only those its digits can reach), digit magnitude m lives in set base[w] + ((m - 1) >> set_log),
// bucket (m - 1) & (2^set_log - 1), and the host gives set j of a window the extra weight j 2^set_log through the set's total (MsmJob::finish).
// Plain C++ (no HIP): the recoder (k_msm_recode_cover, zl_msm_sort.hip), the planner and host finish (zl_msm_job.h) and the stand-alone sanitizer program
// tests/c/msm_cover_plan.cpp share this text -- the split, the digits and the placement are the functions below and nothing else.
//
// Proof obligation of a plan (zl_cover_make checks it from the split's own constants, it is never assumed): |k_i| <= floor(lambda / 2) + 1 (zl_cover_split), so the
// top digit is at most top_live = ((floor(lambda / 2) + 1) >> pos[top]) + 1 (the carry of the window below); top_live must stay BELOW 2^(width[top] - 1), the
// magnitude at which a digit would flip and send a carry out of the top window, and inside the sets the top window owns.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ZL_CV_HD __host__ __device__ __forceinline__
#else
#define ZL_CV_HD inline
#endif

#define ZL_CV_MAX_WINDOWS 8
#define ZL_CV_BITS 128        // what the widths of a plan sum to: the 127 bits of a half-scalar and the carry
#define ZL_CV_GROUP_LOG 15    // buckets per sort group (the three-level sort of zl_msm_sort.hip): the group id travels in a byte, 0xFF = zero digit

struct zl_cover_plan {
    uint32_t windows = 0;   // digits per half-scalar
    uint32_t set_log = 0;   // log2 of the buckets of one device set
    uint32_t nsets = 0;     // device sets of all windows
    uint32_t top_live = 0;  // the largest magnitude the top digit can take
    uint32_t width[ZL_CV_MAX_WINDOWS] = {}, pos[ZL_CV_MAX_WINDOWS] = {};   // bits of window w, and where they start
    uint32_t base[ZL_CV_MAX_WINDOWS] = {}, sets[ZL_CV_MAX_WINDOWS] = {};   // first set of window w, and how many it owns
    uint32_t lambda[4] = {}, barrett[8] = {}, rmod[8] = {};                  // the split: lambda, floor(2^383 / lambda), the group order r = lambda^2 + lambda + 1
};

// failed obligations of zl_cover_make (0 = the plan holds)
enum { ZL_CV_OK = 0, ZL_CV_ESHAPE = 1, ZL_CV_ESUM = 2, ZL_CV_ECARRY = 3, ZL_CV_EGROUPS = 4 };

inline int zl_cover_make(zl_cover_plan& p, const uint32_t* widths, uint32_t windows, uint32_t set_log, const uint32_t lambda[4], const uint32_t barrett[8],
                         const uint32_t rmod[8]) {
    p = zl_cover_plan{};
    if (windows < 1 || windows > ZL_CV_MAX_WINDOWS || set_log < ZL_CV_GROUP_LOG || set_log > 22) return ZL_CV_ESHAPE;
    uint32_t sum = 0;
    for (uint32_t w = 0; w < windows; w++) {
        if (widths[w] < set_log + 1 || widths[w] > 24) return ZL_CV_ESHAPE;  // every window fills whole sets; a digit and its carry fit 25 bits
        p.width[w] = widths[w];
        p.pos[w] = sum;
        sum += widths[w];
    }
    if (sum != ZL_CV_BITS) return ZL_CV_ESUM;
    for (int k = 0; k < 4; k++) p.lambda[k] = lambda[k];
    for (int k = 0; k < 8; k++) { p.barrett[k] = barrett[k]; p.rmod[k] = rmod[k]; }
    p.windows = windows;
    p.set_log = set_log;
    // half_max = floor(lambda / 2) + 1 < 2^127, then its bits from pos[top] on, + 1 for the carry
    uint32_t hm[4];
    for (int k = 0; k < 4; k++) hm[k] = (lambda[k] >> 1) | (k < 3 ? lambda[k + 1] << 31 : 0u);
    for (int k = 0; k < 4; k++) { hm[k] += 1u; if (hm[k] != 0u) break; }
    if (hm[3] >> 31) return ZL_CV_ECARRY;
    const uint32_t top = windows - 1, tp = p.pos[top];
    uint64_t v = 0;  // bits [tp, 128) of hm: at most width[top] <= 24 of them
    for (uint32_t k = 0; k < 4; k++) {
        if (k == (tp >> 5)) v |= hm[k];
        if (k == (tp >> 5) + 1) v |= (uint64_t)hm[k] << 32;
    }
    p.top_live = (uint32_t)(v >> (tp & 31)) + 1u;
    if (p.top_live >= (1u << (p.width[top] - 1))) return ZL_CV_ECARRY;  // the top digit could flip: a carry would leave the scalar
    uint32_t next = 0;
    for (uint32_t w = 0; w < windows; w++) {
        const uint32_t full = 1u << (p.width[w] - 1 - set_log), live = (p.top_live + (1u << set_log) - 1u) >> set_log;
        p.base[w] = next;
        p.sets[w] = w == top ? live : full;  // (live <= full follows from the carry obligation)
        next += p.sets[w];
    }
    p.nsets = next;
    if (((uint64_t)p.nsets << (set_log - ZL_CV_GROUP_LOG)) > 255u) return ZL_CV_EGROUPS;  // 0xFF is the zero digit's group id
    return ZL_CV_OK;
}

// the window that owns device set s (s < nsets)
ZL_CV_HD uint32_t zl_cover_window_of_set(const zl_cover_plan& p, uint32_t s) {
    uint32_t w = 0;
#pragma unroll
    for (uint32_t k = 1; k < ZL_CV_MAX_WINDOWS; k++)
        if (k < p.windows && s >= p.base[k]) w = k;
    return w;
}

// ---- the split: k = k1 + k2 lambda (mod r), |k1|, |k2| <= floor(lambda / 2) + 1.  The arithmetic of k_glv_split (zl_msm_endo.h) on the plan's constants:
// k in [r, 2^255) is reduced once, q = floor(k m / 2^383) with m = floor(2^383 / lambda) is the quotient or one less, then both halves are balanced.
struct zl_cv_u128 { uint64_t lo, hi; };
ZL_CV_HD bool zl_cv_gt(zl_cv_u128 a, zl_cv_u128 b) { return a.hi > b.hi || (a.hi == b.hi && a.lo > b.lo); }
ZL_CV_HD bool zl_cv_ge(zl_cv_u128 a, zl_cv_u128 b) { return a.hi > b.hi || (a.hi == b.hi && a.lo >= b.lo); }
ZL_CV_HD zl_cv_u128 zl_cv_sub(zl_cv_u128 a, zl_cv_u128 b) { return zl_cv_u128{a.lo - b.lo, a.hi - b.hi - (a.lo < b.lo ? 1u : 0u)}; }
ZL_CV_HD zl_cv_u128 zl_cv_inc(zl_cv_u128 a) { return zl_cv_u128{a.lo + 1, a.hi + (a.lo + 1 == 0 ? 1u : 0u)}; }
ZL_CV_HD zl_cv_u128 zl_cv_dec(zl_cv_u128 a) { return zl_cv_u128{a.lo - 1, a.hi - (a.lo == 0 ? 1u : 0u)}; }

// mag1 / mag2: |k1| / |k2| as four words; neg1 / neg2: 1 for a negative (never set on a zero) half
ZL_CV_HD void zl_cover_split(const zl_cover_plan& p, const uint32_t kin[8], uint32_t mag1[4], uint32_t mag2[4], uint32_t& neg1, uint32_t& neg2) {
    uint32_t k[8];
    {
        uint32_t d[8], borrow = 0;
#pragma unroll
        for (int w = 0; w < 8; w++) {
            const uint64_t x = (uint64_t)kin[w] - p.rmod[w] - borrow;
            d[w] = (uint32_t)x;
            borrow = (uint32_t)(x >> 63);
        }
#pragma unroll
        for (int w = 0; w < 8; w++) k[w] = borrow ? kin[w] : d[w];
    }
    uint32_t pw[16];
    {
        uint64_t acc = 0;
        uint32_t top = 0;
#pragma unroll
        for (int col = 0; col < 15; col++) {
#pragma unroll
            for (int a = 0; a < 8; a++) {
                const int b = col - a;
                if (b < 0 || b > 7) continue;
                const uint64_t pr = (uint64_t)k[a] * p.barrett[b];
                acc += pr;
                top += acc < pr ? 1u : 0u;
            }
            pw[col] = (uint32_t)acc;
            acc = (acc >> 32) | ((uint64_t)top << 32);
            top = 0;
        }
        pw[15] = (uint32_t)acc;
    }
    zl_cv_u128 q{((uint64_t)(pw[11] >> 31) | ((uint64_t)pw[12] << 1) | ((uint64_t)pw[13] << 33)), ((uint64_t)(pw[13] >> 31) | ((uint64_t)pw[14] << 1) | ((uint64_t)pw[15] << 33))};
    const uint32_t qw[4] = {(uint32_t)q.lo, (uint32_t)(q.lo >> 32), (uint32_t)q.hi, (uint32_t)(q.hi >> 32)};
    uint32_t t[5];  // q lambda (mod 2^160; k - q lambda is below 2 lambda < 2^129)
    {
        uint64_t acc = 0;
        uint32_t top = 0;
#pragma unroll
        for (int col = 0; col < 5; col++) {
#pragma unroll
            for (int a = 0; a < 4; a++) {
                const int b = col - a;
                if (b < 0 || b > 3) continue;
                const uint64_t pr = (uint64_t)qw[a] * p.lambda[b];
                acc += pr;
                top += acc < pr ? 1u : 0u;
            }
            t[col] = (uint32_t)acc;
            acc = (acc >> 32) | ((uint64_t)top << 32);
            top = 0;
        }
    }
    uint32_t d[5];
    {
        uint32_t borrow = 0;
#pragma unroll
        for (int w = 0; w < 5; w++) {
            const uint64_t x = (uint64_t)k[w] - t[w] - borrow;
            d[w] = (uint32_t)x;
            borrow = (uint32_t)(x >> 63);
        }
    }
    const zl_cv_u128 LAM{(uint64_t)p.lambda[0] | ((uint64_t)p.lambda[1] << 32), (uint64_t)p.lambda[2] | ((uint64_t)p.lambda[3] << 32)};
    const zl_cv_u128 HALF{(LAM.lo >> 1) | (LAM.hi << 63), LAM.hi >> 1};
    zl_cv_u128 k1{(uint64_t)d[0] | ((uint64_t)d[1] << 32), (uint64_t)d[2] | ((uint64_t)d[3] << 32)};
    uint32_t k1top = d[4];
#pragma unroll
    for (int rep = 0; rep < 2; rep++) {
        if (k1top != 0u || zl_cv_ge(k1, LAM)) {
            const bool br = zl_cv_gt(LAM, k1);
            k1 = zl_cv_sub(k1, LAM);
            k1top -= br ? 1u : 0u;
            q = zl_cv_inc(q);
        }
    }
    zl_cv_u128 k2 = q;
    neg1 = 0;
    neg2 = 0;
    if (zl_cv_gt(k1, HALF)) { k1 = zl_cv_sub(LAM, k1); neg1 = 1; k2 = zl_cv_inc(k2); }
    if (zl_cv_gt(k2, HALF)) {
        k2 = zl_cv_sub(zl_cv_inc(LAM), k2);
        neg2 = 1;
        if (neg1) k1 = zl_cv_inc(k1);
        else if ((k1.lo | k1.hi) == 0) { k1.lo = 1; neg1 = 1; }
        else k1 = zl_cv_dec(k1);
    }
    if ((k1.lo | k1.hi) == 0) neg1 = 0;
    if ((k2.lo | k2.hi) == 0) neg2 = 0;
    mag1[0] = (uint32_t)k1.lo; mag1[1] = (uint32_t)(k1.lo >> 32); mag1[2] = (uint32_t)k1.hi; mag1[3] = (uint32_t)(k1.hi >> 32);
    mag2[0] = (uint32_t)k2.lo; mag2[1] = (uint32_t)(k2.lo >> 32); mag2[2] = (uint32_t)k2.hi; mag2[3] = (uint32_t)(k2.hi >> 32);
}

// ---- the digits of one half: sum_w (neg_w ? -m_w : m_w) 2^pos[w] = (sg ? -mag : mag), 0 <= m_w <= 2^(width[w] - 1).
// One step of the walk, windows taken low to high with carry = 0 at the start.  Tie at d = 2^(width - 1): kept for a positive half, flipped (with a carry) for a
// negative one, whose digits all change sign below -- so the magnitude 2^(width - 1) only ever ends up with a clear sign (the rule of k_msm_recode).
// neg is the FINAL sign of the digit (the half's sign folded in); m = 0: no entry.
ZL_CV_HD void zl_cover_digit(const zl_cover_plan& p, const uint32_t mag[4], uint32_t sg, uint32_t w, uint32_t& carry, uint32_t& m, uint32_t& neg) {
    const uint32_t pos = p.pos[w], width = p.width[w], word = pos >> 5, sh = pos & 31;
    uint64_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {  // register-resident select instead of a dynamically indexed array
        if (k == word) v |= mag[k];
        if (k == word + 1) v |= (uint64_t)mag[k] << 32;
    }
    uint32_t d = ((uint32_t)(v >> sh) & ((1u << width) - 1u)) + carry;
    const uint32_t Hw = 1u << (width - 1);
    uint32_t flip = 0;
    carry = 0;
    if (d > Hw - sg) { d = 2u * Hw - d; flip = 1; carry = 1; }
    m = d;
    neg = d ? (flip ^ sg) : 0u;
}
// ... and whether the walk ended inside the plan: no carry out of the top window, the top digit within its live range.  A half within the split's bound always
// does (zl_cover_make); anything else is reported, never wrapped.
ZL_CV_HD bool zl_cover_top_ok(const zl_cover_plan& p, uint32_t top_m, uint32_t carry_out) { return carry_out == 0u && top_m <= p.top_live; }

// where digit magnitude m >= 1 of window w lives: device set and bucket inside it; the bucket's weight inside the set is bucket + 1, the set's extra weight
// (set - base[w]) 2^set_log
ZL_CV_HD void zl_cover_place(const zl_cover_plan& p, uint32_t w, uint32_t m, uint32_t& set, uint32_t& bucket) {
    set = p.base[w] + ((m - 1u) >> p.set_log);
    bucket = (m - 1u) & ((1u << p.set_log) - 1u);
}
