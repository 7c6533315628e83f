// msm_cover_plan.cpp -- stand-alone walk of the exact-cover window plan (openzl_amd/csrc/zl_msm_cover_plan.h) on the host, built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_msm_cover_plan.py.  The header is the text the recoder kernel, the planner and the host finish compile; this program
// checks, with its own multi-word arithmetic, that
//   - the constants are what they claim (r = lambda^2 + lambda + 1, barrett = floor(2^383 / lambda)) and zl_cover_make accepts exactly the plans whose obligations hold;
//   - k1 + k2 lambda = k (mod r) with |k_i| <= floor(lambda / 2) + 1 for every scalar;
//   - sum_w (+-m_w) 2^pos[w] reproduces each half, m_w <= 2^(width - 1), the tie magnitude only ever carries a clear sign, the top digit stays inside its live range
//     with no carry out, and every digit's (set, bucket) lies inside the sets its window owns, weighs what the digit says and has a sort group id below 0xFF;
// on k in {0, 1, 2, r - 1, r - 2}, halves at +- their maximum, every window at the tie 2^(w - 1) and one either side of it, carry chains through all windows and 10^5
// random scalars, for the 22/21/21/21/21/22 plan of 2^24 points and a seven-window plan (19/18/18/18/18/18/19 over sets of 2^17).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "zl_msm_cover_plan.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                                    \
    do {                                                                    \
        if (!(cond)) {                                                      \
            if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
            g_fail++;                                                       \
        }                                                                   \
    } while (0)

// ---- 512-bit unsigned integers, 16 words
struct Big { uint32_t w[16]; };
static Big big0() { Big b; memset(&b, 0, sizeof b); return b; }
static Big big_words(const uint32_t* p, int n) { Big b = big0(); for (int i = 0; i < n; i++) b.w[i] = p[i]; return b; }
static Big big_u(uint64_t v) { Big b = big0(); b.w[0] = (uint32_t)v; b.w[1] = (uint32_t)(v >> 32); return b; }
static Big add(const Big& a, const Big& b) { Big r; uint64_t c = 0; for (int i = 0; i < 16; i++) { c += (uint64_t)a.w[i] + b.w[i]; r.w[i] = (uint32_t)c; c >>= 32; } return r; }
static Big sub(const Big& a, const Big& b) { Big r; uint64_t br = 0; for (int i = 0; i < 16; i++) { const uint64_t x = (uint64_t)a.w[i] - b.w[i] - br; r.w[i] = (uint32_t)x; br = (x >> 63) & 1u; } return r; }
static int cmp(const Big& a, const Big& b) { for (int i = 15; i >= 0; i--) if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1; return 0; }
static Big mul(const Big& a, const Big& b) {  // low 512 bits
    Big r = big0();
    for (int i = 0; i < 16; i++) {
        uint64_t c = 0;
        for (int j = 0; i + j < 16; j++) { c += (uint64_t)a.w[i] * b.w[j] + r.w[i + j]; r.w[i + j] = (uint32_t)c; c >>= 32; }
    }
    return r;
}
static Big shl(const Big& a, unsigned s) {
    Big r = big0();
    const unsigned ws = s >> 5, bs = s & 31;
    for (int i = 15; i >= (int)ws; i--) {
        uint64_t v = (uint64_t)a.w[i - ws] << bs;
        if (bs && i - (int)ws - 1 >= 0) v |= a.w[i - ws - 1] >> (32 - bs);
        r.w[i] = (uint32_t)v;
    }
    return r;
}
static Big mod(Big a, const Big& m) { int guard = 0; while (cmp(a, m) >= 0 && guard++ < 64) a = sub(a, m); return a; }  // (operands are a few multiples of m at most)

// BLS12-381: lambda = z^2 - 1, floor(2^383 / lambda), r (what gen_params.py writes into zl_params.h; verified below, not trusted)
static const uint32_t LAMBDA[4] = {0xffffffffu, 0x00000000u, 0x0001a402u, 0xac45a401u};
static const uint32_t BARRETT[8] = {0xc4b6396eu, 0xed2f27c6u, 0x9345fbd1u, 0x1c4fa4d3u, 0x7b67f718u, 0xb1fb7291u, 0xf00fd56eu, 0xbe35f678u};
static const uint32_t RMOD[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
static Big LAM, R, HALFMAX;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27; return g_rng * 0x2545F4914F6CDD1Dull; }

struct Stats { uint64_t digits = 0, ties = 0, carries_into_top = 0; uint32_t top_max = 0; };

// the digits of one half against the plan: the sum, the bounds, the placement.  expect_ok = false: the half is outside the split's bound and the walk must say so.
static void walk_half(const zl_cover_plan& p, const uint32_t mag[4], uint32_t sg, bool expect_ok, Stats& st) {
    Big pos = big0(), neg = big0();
    uint32_t carry = 0, m = 0, ng = 0;
    const uint32_t gshift = p.set_log - ZL_CV_GROUP_LOG;
    for (uint32_t w = 0; w < p.windows; w++) {
        const uint32_t carry_in = carry;
        zl_cover_digit(p, mag, sg, w, carry, m, ng);
        const uint32_t Hw = 1u << (p.width[w] - 1);
        CHECK(m <= Hw, "digit %u above half its window", m);
        CHECK(ng <= 1u && (m != 0u || ng == 0u), "sign of a zero digit");
        if (m == Hw) { CHECK(ng == 0u, "tie magnitude with the sign set (window %u)", w); st.ties++; }
        if (w + 1 == p.windows) {
            const bool ok = zl_cover_top_ok(p, m, carry);
            CHECK(ok == expect_ok, "top digit %u carry %u: ok = %d, expected %d", m, carry, (int)ok, (int)expect_ok);
            if (!ok) return;  // the recoder drops the entry and flags the job
            if (m > st.top_max) st.top_max = m;
            st.carries_into_top += carry_in;
        }
        if (m) {
            uint32_t set, bucket;
            zl_cover_place(p, w, m, set, bucket);
            CHECK(set >= p.base[w] && set < p.base[w] + p.sets[w] && set < p.nsets, "set %u outside window %u", set, w);
            CHECK(bucket < (1u << p.set_log), "bucket %u", bucket);
            CHECK((((uint64_t)(set - p.base[w])) << p.set_log) + bucket + 1u == m, "weight of (set %u, bucket %u) is not %u", set, bucket, m);
            CHECK(zl_cover_window_of_set(p, set) == w, "window of set %u", set);
            CHECK(((set << gshift) | (bucket >> ZL_CV_GROUP_LOG)) < 255u, "group id");
            const Big term = shl(big_u(m), p.pos[w]);
            if (ng) neg = add(neg, term); else pos = add(pos, term);
            st.digits++;
        }
    }
    const Big M = big_words(mag, 4);
    if (sg) CHECK(cmp(neg, add(pos, M)) == 0, "digits do not sum to -half");
    else CHECK(cmp(pos, add(neg, M)) == 0, "digits do not sum to +half");
}

static void check_scalar(const zl_cover_plan& p, const Big& k, Stats& st) {
    uint32_t mag1[4], mag2[4], n1 = 7, n2 = 7;
    zl_cover_split(p, k.w, mag1, mag2, n1, n2);
    const Big K1 = big_words(mag1, 4), K2 = big_words(mag2, 4);
    CHECK(n1 <= 1u && n2 <= 1u, "signs");
    CHECK(cmp(K1, HALFMAX) <= 0 && cmp(K2, HALFMAX) <= 0, "a half above floor(lambda / 2) + 1");
    CHECK(!(n1 && cmp(K1, big0()) == 0) && !(n2 && cmp(K2, big0()) == 0), "negative zero");
    // k1 + k2 lambda = k (mod r): positive terms on one side, negative ones on the other
    Big lhs = mod(k, R), rhs = big0();
    const Big t2 = mul(K2, LAM);
    if (n1) lhs = add(lhs, K1); else rhs = add(rhs, K1);
    if (n2) lhs = add(lhs, t2); else rhs = add(rhs, t2);
    CHECK(cmp(mod(lhs, R), mod(rhs, R)) == 0, "k1 + k2 lambda != k (mod r)");
    walk_half(p, mag1, n1, true, st);
    walk_half(p, mag2, n2, true, st);
}

// k = s1 a + s2 b lambda (mod r) for chosen halves
static Big compose(const Big& a, int s1, const Big& b, int s2) {
    Big pos = big0(), neg = big0();
    const Big t = mod(mul(b, LAM), R);
    if (s1 >= 0) pos = add(pos, a); else neg = add(neg, a);
    if (s2 >= 0) pos = add(pos, t); else neg = add(neg, t);
    return mod(sub(add(pos, add(R, R)), neg), R);
}

static void run_plan(const uint32_t* widths, uint32_t windows, uint32_t set_log, uint32_t want_sets) {
    zl_cover_plan p;
    const int rc = zl_cover_make(p, widths, windows, set_log, LAMBDA, BARRETT, RMOD);
    CHECK(rc == ZL_CV_OK, "zl_cover_make: %d", rc);
    if (rc != ZL_CV_OK) return;
    CHECK(p.nsets == want_sets, "%u sets, expected %u", p.nsets, want_sets);
    uint32_t sum = 0;
    for (uint32_t w = 0; w < windows; w++) { CHECK(p.pos[w] == sum, "pos"); sum += p.width[w]; }
    CHECK(sum == 128, "widths sum to %u", sum);
    const uint32_t top = windows - 1;
    // the obligation, recomputed here: ((floor(lambda / 2) + 1) >> pos[top]) + 1 < 2^(width[top] - 1), inside the owned sets
    {
        Big h = HALFMAX;
        for (uint32_t s = 0; s < p.pos[top]; s++) { for (int i = 0; i < 15; i++) h.w[i] = (h.w[i] >> 1) | (h.w[i + 1] << 31); h.w[15] >>= 1; }
        CHECK(h.w[1] == 0 && h.w[0] + 1u == p.top_live, "top_live %u", p.top_live);
        CHECK(p.top_live < (1u << (p.width[top] - 1)), "the top digit could flip");
        CHECK(p.top_live <= (p.sets[top] << set_log) && p.top_live > ((p.sets[top] - 1) << set_log), "sets of the top window");
    }
    Stats st;
    // edge scalars
    const Big one = big_u(1), two = big_u(2);
    const Big edge[5] = {big0(), one, two, sub(R, one), sub(R, two)};
    for (const Big& k : edge) check_scalar(p, k, st);
    // scalars in [r, 2^255): reduced once by the split
    check_scalar(p, R, st);
    check_scalar(p, add(R, big_u(12345)), st);
    { Big k = big0(); for (int i = 0; i < 8; i++) k.w[i] = 0xFFFFFFFFu; k.w[7] = 0x7FFFFFFFu; check_scalar(p, k, st); }
    // halves at +- their maximum (and one inside it)
    const Big hm1 = sub(HALFMAX, one);
    for (int s1 = -1; s1 <= 1; s1 += 2)
        for (int s2 = -1; s2 <= 1; s2 += 2)
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) {
                    const Big A = a == 0 ? HALFMAX : (a == 1 ? hm1 : big0()), B = b == 0 ? HALFMAX : (b == 1 ? hm1 : big0());
                    check_scalar(p, compose(A, s1, B, s2), st);
                }
    // every window at the tie 2^(w - 1) and one either side, both signs, with nothing / all ones / random bits below; in the top window those magnitudes are
    // outside the split's bound: the walk must report them.  Directly on the digits, and through the split (k = +-half, which splits to (half, 0) below the top).
    for (uint32_t w = 0; w < windows; w++)
        for (int delta = -1; delta <= 1; delta++)
            for (uint32_t sg = 0; sg < 2; sg++)
                for (int low = 0; low < 3; low++) {
                    const uint32_t d = (1u << (p.width[w] - 1)) + (uint32_t)delta;
                    Big M = shl(big_u(d), p.pos[w]);
                    if (low && p.pos[w]) {
                        Big below = sub(shl(one, p.pos[w]), one);
                        if (low == 2) for (int i = 0; i < 4; i++) below.w[i] &= (uint32_t)rnd();
                        M = add(M, below);
                    }
                    // (all ones below can carry into the field: the digit then sits one higher, which is the other side of the tie).  Below the top window every such
                    // half is inside the split's bound; in the top window none is, and its top digit is outside the live range whatever the sign
                    const bool in_bound = cmp(M, HALFMAX) <= 0;
                    CHECK(in_bound == (w != top), "bound of a tie half");
                    const bool expect_ok = in_bound;
                    walk_half(p, M.w, sg, expect_ok, st);
                    if (in_bound) {
                        check_scalar(p, compose(M, sg ? -1 : 1, big0(), 1), st);
                        check_scalar(p, compose(big0(), 1, M, sg ? -1 : 1), st);
                    }
                }
    CHECK(st.ties > 0, "no tie digit was met");
    // a top field beyond the live range and a carry out of the top window are reported, not wrapped
    {
        Stats tmp;
        uint32_t M[4] = {0, 0, 0, 0x80000000u};  // 2^127: the top field is 2^(width - 1)
        walk_half(p, M, 0, false, tmp);
        walk_half(p, M, 1, false, tmp);
        uint32_t F[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};  // every digit flips, the carry leaves the scalar
        walk_half(p, F, 0, false, tmp);
        Big L = shl(big_u(p.top_live + 1u), p.pos[top]);  // one above the live range
        walk_half(p, L.w, 0, false, tmp);
        Big L0 = shl(big_u(p.top_live), p.pos[top]);      // the live range's last magnitude itself is placed
        walk_half(p, L0.w, 1, true, tmp);
    }
    // carry chains through all windows: every field below the top at all ones (each digit flips and carries), at half + 1 in window 0 and exactly half above
    // (the carry lifts every later field over the tie), alternating, both signs, through the digits and through the split
    for (uint32_t t = 0; t < 4; t++)
        for (uint32_t sg = 0; sg < 2; sg++) {
            Big chains[3];
            chains[0] = add(shl(big_u(t), p.pos[top]), sub(shl(one, p.pos[top]), one));
            chains[1] = shl(big_u(t), p.pos[top]);
            chains[2] = shl(big_u(t), p.pos[top]);
            for (uint32_t w = 0; w < top; w++) {
                const uint32_t Hw = 1u << (p.width[w] - 1);
                chains[1] = add(chains[1], shl(big_u(w == 0 ? Hw + 1u : Hw), p.pos[w]));
                chains[2] = add(chains[2], shl(big_u((w & 1) ? 2u * Hw - 1u : Hw + 1u), p.pos[w]));
            }
            for (const Big& M : chains) {
                Stats before = st;
                walk_half(p, M.w, sg, true, st);
                CHECK(st.carries_into_top == before.carries_into_top + 1, "the chain did not carry into the top window");
                check_scalar(p, compose(M, sg ? -1 : 1, big0(), 1), st);
                check_scalar(p, compose(hm1, 1, M, sg ? -1 : 1), st);
            }
        }
    // random scalars below r
    for (int it = 0; it < 100000; it++) {
        Big k = big0();
        for (int i = 0; i < 4; i++) { const uint64_t v = rnd(); k.w[2 * i] = (uint32_t)v; k.w[2 * i + 1] = (uint32_t)(v >> 32); }
        k.w[7] &= 0x7FFFFFFFu;
        check_scalar(p, mod(k, R), st);
    }
    CHECK(st.top_max <= p.top_live, "top digit %u above its live range %u", st.top_max, p.top_live);
    printf("plan %u windows, %u sets of 2^%u: %llu digits, %llu ties, top digit <= %u (live range %u)\n", windows, p.nsets, set_log, (unsigned long long)st.digits,
           (unsigned long long)st.ties, st.top_max, p.top_live);
}

int main() {
    LAM = big_words(LAMBDA, 4);
    R = big_words(RMOD, 8);
    const Big one = big_u(1);
    // the constants: r = lambda^2 + lambda + 1; barrett lambda <= 2^383 < (barrett + 1) lambda
    CHECK(cmp(R, add(add(mul(LAM, LAM), LAM), one)) == 0, "r != lambda^2 + lambda + 1");
    {
        const Big B = big_words(BARRETT, 8), P2 = shl(one, 383);
        CHECK(cmp(mul(B, LAM), P2) <= 0 && cmp(mul(add(B, one), LAM), P2) > 0, "barrett != floor(2^383 / lambda)");
    }
    {   // floor(lambda / 2) + 1
        Big h = LAM;
        for (int i = 0; i < 15; i++) h.w[i] = (h.w[i] >> 1) | (h.w[i + 1] << 31);
        h.w[15] >>= 1;
        HALFMAX = add(h, one);
    }
    const uint32_t w6[6] = {22, 21, 21, 21, 21, 22};
    run_plan(w6, 6, 19, 15);
    const uint32_t w7[7] = {19, 18, 18, 18, 18, 18, 19};
    run_plan(w7, 7, 17, 2 + 5 * 1 + 2);
    // plans whose obligations do not hold are refused
    {
        zl_cover_plan p;
        const uint32_t short_sum[6] = {21, 21, 21, 21, 21, 22}, wide15[6] = {24, 24, 20, 20, 20, 20}, narrow[7] = {22, 21, 21, 21, 21, 12, 10};
        const uint32_t big_lambda[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, full_lambda[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFF0u};
        CHECK(zl_cover_make(p, short_sum, 6, 19, LAMBDA, BARRETT, RMOD) == ZL_CV_ESUM, "a plan of 127 bits was accepted");
        CHECK(zl_cover_make(p, wide15, 6, 15, LAMBDA, BARRETT, RMOD) == ZL_CV_EGROUPS, "more than 255 sort groups were accepted");
        CHECK(zl_cover_make(p, narrow, 7, 19, LAMBDA, BARRETT, RMOD) == ZL_CV_ESHAPE, "a window below one set was accepted");
        CHECK(zl_cover_make(p, w6, 9, 19, LAMBDA, BARRETT, RMOD) == ZL_CV_ESHAPE, "nine windows were accepted");
        CHECK(zl_cover_make(p, w6, 6, 19, big_lambda, BARRETT, RMOD) == ZL_CV_ECARRY, "halves of 128 bits were accepted");
        CHECK(zl_cover_make(p, w6, 6, 19, full_lambda, BARRETT, RMOD) == ZL_CV_ECARRY, "a top digit that can flip was accepted");
    }
    if (g_fail) { printf("msm_cover_plan: %d FAILED\n", g_fail); return 1; }
    printf("msm_cover_plan: OK\n");
    return 0;
}
