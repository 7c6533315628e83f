/* zl_backend_test.h -- TEST-ONLY hooks of libzl_backend.so (not part of the drop-in boundary of zl_backend.h).
 *
 * They expose the device (and host) field / group arithmetic below the MSM / NTT entry points so that tests can
 *   - pin the device Montgomery multiplier to the one known-answer vector the reference holds: the Poseidon permutation of
 *     [3, 1, 2] over BLS12-381 Fr (/root/reference/openzl-tutorials/src/poseidon.rs:364-405, same numbers in
 *     /root/reference/plugins/arkworks/src/poseidon/permutation_hardcoded_test/width3), and
 *   - drive the lazily reduced 14 x 28-bit field (openzl_amd/csrc/zl_field28.h) and the point formulas built on it with operands AT
 *     their contract bounds, which random MSM inputs never produce, and
 *   - drive the LANE FORMS of that arithmetic the same way: Fq2 split over a lane pair (openzl_amd/csrc/zl_fq2pair.h, Fp2H) and one XYZZ addition over the
 *     four lanes of a quad / the eight lanes of an octet (openzl_amd/csrc/zl_quad.h), placed on lanes and in memory exactly as the MSM kernels place them.
 * Nothing in the product path calls them.
 */
#ifndef ZL_BACKEND_TEST_H
#define ZL_BACKEND_TEST_H
#include "zl_backend_ext.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Poseidon permutation, width 3, tutorial schedule (8 full + 55 partial rounds, x^5), computed ON THE DEVICE by one wavefront with
 * the device Fr multiplier the NTT uses; round constants / MDS come from the host mirror (Grain LFSR, Cauchy matrix).
 * state: 3 x 4 u64 canonical, in place.  All 64 lanes compute the same permutation; ZL_EHIP if they disagree. */
int zl_test_poseidon_permute_dev(zl_ctx* ctx, zl_curve_t curve, uint64_t* state);
/* The same permutation computed with the lazily reduced Fr multiplier of the NTT PASSES (openzl_amd/csrc/zl_field28r.h): since round 5 nine 29-bit limbs
 * (mul29r_asm, R' = 2^261) -- and, in the same call, round 4's ten 28-bit limbs (mul28r_asm, R' = 2^280); the two must agree:
 * since round 4 the hot NTT no longer multiplies with the 8 x 32 carry chain the hook above exercises, so the reference's [3, 1, 2] vector is run
 * through this multiplier as well (conversions, 63 rounds, Fermat inversions for the MDS entries, lazy additions without comparisons, one canon at the end). */
int zl_test_poseidon_permute_dev28r(zl_ctx* ctx, zl_curve_t curve, uint64_t* state);

/* Raw-limb access to the 14 x 28-bit BLS12-381 Fq (values are NOT reduced: the caller chooses them anywhere inside a contract).
 * ctx == NULL runs the host code path (7 x 56-bit fast path), otherwise the device path (inline-asm product scans).
 * in: n records of 4 operands (a, b, c, d) x 14 u32 limbs; out: n x 14 u32 limbs (predicates: out[0] = 0 / 1).
 * op: 0 mul(a,b)  1 sqr(a)  2 muladd(a,b,c,d)  3 add(a,b)  4 dbl(a)  5..10 subk<1..6>(a,b)  11 wred(a)  12 canon(a)
 *     13 is_zero(a)  14 a == b  15 muladd4(a,b,c,d,a,d,c,b)  16 load_mont32 . store_canon round trip is op 17/18:
 *     17 load_canon(12 words in a) -> limbs   18 store_canon(a) -> 12 words
 *     scan-only operand forms (un-carried on the device, zl_field28.h subk_scan / negk_scan / x3_of; b, c, d carried, c, d < 8q in op 19, a < 2q in op 20):
 *     19 muladd(a, b - c + 16q, 16q - d, a)   20 mul(4q - a, b)   21 a - b - 2c + 6q (b, c < 2^28 per limb) */
int zl_test_fp28_op(zl_ctx* ctx, int op, const uint32_t* in, size_t n, uint32_t* out);
/* The same operations on the 10-limb BN254 base field (round 4: Fp28<BN254_Fq28, BN254_Fq>, R' = 2^280): records of 4 operands x 10 u32 limbs -> 10 limbs;
 * ops 17 / 18 move 8 canonical words.  (muladd4 and the Fq2 helpers are not used by BN254 G1; op 15 still computes.) */
int zl_test_fp28_bn_op(zl_ctx* ctx, int op, const uint32_t* in, size_t n, uint32_t* out);

/* Raw-limb access to the fully reduced carry-chain field Fp<P> (openzl_amd/csrc/zl_field.h: N words of 32 bits, R = 2^(32 N)) and to Fp2<P> over it
 * (zl_curve.h, Fq[u] / (u^2 + 1)).  No conversion and no reduction happens on the way in: the caller places operands anywhere in N words, at or above p included.
 * field: 0 BLS12-381 Fr (N = 8)  1 BLS12-381 Fq (N = 12)  2 BN254 Fr (N = 8)  3 BN254 Fq (N = 8)
 * form:  the multiplier under every op that multiplies:  0 zl::mul / zl::sqr as the hook's unit builds them (device: the out-of-line call, host: the
 *        64-bit-limb loop)  1 mul_impl directly (device: the product scan inlined, as the Poseidon, NTT and G1 units compile it)  2 the portable 32-bit loop mul_body
 * in:    n records of four operands a, b, c, d x N words; out: n x N words (predicates: 0 / 1 in word 0, the other words 0), Fp2 ops n x 2 N words
 * op:    0 mul(a,b)  1 sqr(a)  2 add(a,b)  3 sub(a,b)  4 dbl(a)  5 neg(a)  6 to_mont(a)  7 from_mont(a)  8 inv(a)  9 a.is_zero()  10 a == b
 *        11 reduce_once(a) (a < 2p)  12 from_u64(a.l[0] | a.l[1] << 32)
 *        Fp2, fields 1 and 3 only, x = (a, b), y = (c, d):  20 mul(x,y)  21 sqr(x)  22 inv(x)  23 add(x,y)  24 sub(x,y)  25 neg(x)  26 to_mont(x)  27 from_mont(x)
 * ctx == NULL runs the host code, otherwise one lane per record in blocks of 64.  ZL_EINVAL: an unknown field, form or op, an Fp2 op on a scalar field, a null
 * pointer with n > 0, n >= 2^24. */
int zl_test_fp_op(zl_ctx* ctx, int field, int form, int op, const uint32_t* in, size_t n, uint32_t* out);

/* Point formulas of zl_curve.h over that field.  group: ZL_G1 (coordinate = 14 words) or ZL_G2 (coordinate = 2 x 14 words);
 * hot != 0 selects, for G2, the flavour with inlined product scans that the bucket accumulation kernel uses.
 * in: n records of two XYZZ points p, q (x, y, zz, zzz each), raw limbs, zz == 0 encodes infinity; out: n XYZZ points.
 * op: 0 add_mixed(p, q.x, q.y, +)  1 add_mixed(p, q.x, q.y, -)  2 add_full(p, q)  3 dbl_inplace(p)  4 dbl_affine(p.x, p.y)
 *     5 neg_inplace(p)  6 to_affine(p) (x, y in the first two coordinates) */
int zl_test_point_op(zl_ctx* ctx, zl_group_t group, int hot, int op, const uint32_t* in, size_t n, uint32_t* out);

/* Fq2 over a LANE PAIR (Fp2H of openzl_amd/csrc/zl_fq2pair.h: c0 in lane i, c1 in lane i ^ 8 of a row of 16), device only: a null ctx is ZL_EINVAL.
 * curve: ZL_BLS12_381 (L = 14 limbs per component) or ZL_BN254 (L = 10).  in: n records of 4 Fq2 operands (a, b, c, d), each c0 || c1 as 2 x L raw limbs
 * (NOT reduced: the caller chooses them anywhere inside a contract); out: n x 2 L limbs.  The kernel maps lanes to records with ZL_PAIR_ITEM / pair_half and
 * moves operands with pair_load / pair_store, on the memory layout of the product (two 64-byte components per element): 32 records per wave.
 * op: 0 mul(a,b)  1 sqr(a)  2 muladd(a,b,c,d)  3 add(a,b)  4 dbl(a)  5..10 subk<1..6>(a,b)  11 wred(a)  12 canon(a)
 *     13 is_zero(a)  14 raw_zero(a) (predicates: 0 / 1 in limb 0 of BOTH components, the other limbs 0)  15 x3_of(a,b,c) = a - b - 2c + 6q
 *     16 Fp2H::one()  17..22 negk<1..6>(a) */
int zl_test_fp2pair_op(zl_ctx* ctx, zl_curve_t curve, int op, const uint32_t* in, size_t n, uint32_t* out);

/* The point formulas in every form the kernels run them in.  Records, op numbers and meaning as zl_test_point_op; a coordinate is L words (G1) or 2 L words (G2),
 * L = 14 for ZL_BLS12_381 and 10 for ZL_BN254.
 *   ZL_TEST_FORM_SCALAR / _SCALAR_HOT  one lane per item, the called / the inlined Fq2 flavour (G1: the same code); host path with a null ctx
 *   ZL_TEST_FORM_QUAD    G1 only: four lanes per item, ops 0-2 through add_mixed_quad / add_full_quad, 3-6 by every lane on its own; 16 items per wave
 *   ZL_TEST_FORM_PAIR    G2 only: Fp2H, the per-lane formulas on a lane pair, items by ZL_PAIR_ITEM, pair_load / pair_store; 32 items per wave
 *   ZL_TEST_FORM_OCTET   G2 only: add_*_quad over Fp2H (ops 0-2; 3-5 per lane pair), items by ZL_OCTET_ITEM; 8 items per wave
 * The three lane forms run on the device only (null ctx: ZL_EINVAL); a group a form does not exist for is ZL_EINVAL, and so is op 6 on PAIR / OCTET
 * (Fp2H has no inversion: no kernel leaves the XYZZ form on lane pairs).  QUAD / OCTET: lane 0 of each quad stores the result, and ZL_EHIP is returned
 * if the four lanes of any quad (each of the two quads of an octet) did not end with identical limbs. */
typedef enum { ZL_TEST_FORM_SCALAR = 0, ZL_TEST_FORM_SCALAR_HOT = 1, ZL_TEST_FORM_QUAD = 2, ZL_TEST_FORM_PAIR = 3, ZL_TEST_FORM_OCTET = 4 } zl_test_form_t;
int zl_test_point_form_op(zl_ctx* ctx, zl_curve_t curve, zl_group_t group, int form, int op, const uint32_t* in, size_t n, uint32_t* out);

/* Turns `c` into a different circuit of the SAME shape (the first coefficient of row 0 of A is doubled; the assignment no longer satisfies
 * it).  A proving context compiled for / bound to the original circuit must refuse the tweaked one (its matrices are device-resident and are
 * not re-uploaded per proof): zl_groth16_prove_circuit returns ZL_EINVAL instead of proving against the wrong matrices. */
int zl_test_circuit_tweak(zl_circuit* c);

/* The lazily reduced 10 x 28-bit scalar field of the NTT passes (openzl_amd/csrc/zl_field28r.h), host (ctx == NULL) or device (inline-asm product scan).
 * in: n records of two values a, b as 8 u32 words each (any value < 2^256); out: n x 8 words, always the canonical result.  j = log2 of the bias
 * multiple of r used by the subtractions (0..20).  op: 0 mul(a, b) (= a b 2^-280 mod r)  1 a + b  2 a - b  3 canon(a)  4 a chain of lazy
 * additions / biased subtractions at the bounds the passes reach, closed by one product (zl_testhooks.hip). */
int zl_test_fr28_op(zl_ctx* ctx, zl_curve_t curve, int op, int j, const uint32_t* in, size_t n, uint32_t* out);
/* The same header instantiated on NINE limbs of 29 bits (round 5: *_Fr29, R' = 2^261, what the NTT passes multiply with): op 0 = a b 2^-261 mod r; j <= 6; the
 * chain of op 4 weakly reduces after every step (its products only take B(a) B(b) <= 70 / 169); op 5 (both instances) canon(wred(2a + 2b)). */
int zl_test_fr29_op(zl_ctx* ctx, zl_curve_t curve, int op, int j, const uint32_t* in, size_t n, uint32_t* out);

/* MEASUREMENT ONLY (bench.py's integer-ALU roofline): chains of the accumulation kernel's 14 x 28-bit Montgomery product on per-lane pseudo-random
 * operands, cu_count x 4 x waves_per_simd wavefronts, `iters` products per lane; returns 10^9 products per second.  This is the live-data ceiling of
 * the multiplier on the box of the run (constant-pattern operands run 11 % faster, short launches after an idle gap 10-15 % slower: time >= 0.1 s after a
 * warm-up; profiles/r04_fbench_f64.log). */
int zl_test_fq_mul_rate(zl_ctx* ctx, int waves_per_simd, int iters, double* g_products_per_s);

/* MEASUREMENT ONLY: the effective shader clock of the two integer bodies the rooflines are quoted against (MI355X clocks dense VALU bodies to its power
 * budget; VERDICT r4 missing #2).  Every wave reads s_memtime (shader cycles) and s_memrealtime (constant 100 MHz) at its start and end; the clock is
 * the sum of cycle deltas over the sum of tick deltas.  out[0] effective GHz, out[1] span of the launch in ms by the tick counter, out[2] waves,
 * out[3] mean life of a wave in ms, out[4] / out[5] smallest / largest per-wave GHz.
 *   zl_test_fq_mul_clock: the multiplier chain of zl_test_fq_mul_rate; additionally out[6] = 10^9 products/s and out[7] = ms by HIP events (out: 8 doubles).
 *   zl_test_acc_clock(ctx, 1) arms the ctx: every following LARGE G1 bucket accumulation (one lane per chunk) of this ctx runs as k_msm_accumulate_clk -- the
 *   product kernel plus those four scalar reads per wave; zl_test_acc_clock_read reduces the records of the last such launch (out: 6 doubles);
 *   zl_test_acc_clock(ctx, 0) disarms and frees. */
int zl_test_fq_mul_clock(zl_ctx* ctx, int waves_per_simd, int iters, double* out);
int zl_test_acc_clock(zl_ctx* ctx, int on);
int zl_test_acc_clock_read(zl_ctx* ctx, double* out);
/* ... and for kernels without instrumentation (the NTT passes): zl_test_clock_probe_launch starts eight one-wave blocks (one per XCD) on a stream of their
 * own that sleep-spin on the 100-MHz counter for spin_us microseconds; launch it right before the work to observe, run the work, then
 * zl_test_clock_probe_read (out: 6 doubles as above) = the effective clock of the chip during that window. */
int zl_test_clock_probe_launch(zl_ctx* ctx, unsigned spin_us);
int zl_test_clock_probe_read(zl_ctx* ctx, double* out);

/* prod_i e(P_i, Q_i), n <= 64 pairs (P_i: x || y canonical u64 words, Q_i: x.c0 || x.c1 || y.c0 || y.c1; all-zero = infinity), after ONE final exponentiation:
 * the lock-step Miller loops of Groth16::verify (csrc/zl_pairing.h miller_multi), 12 canonical Fq coefficients as zl_pairing. */
int zl_test_pairing_product(zl_curve_t curve, size_t n, const uint64_t* ps_xy, const uint64_t* qs_xy, uint64_t* out12);

/* The device Miller loops of zl_pairing_product, one value per pair: out = n x 12 canonical Fq coefficients (BLS12-381: 12 x 6 u64, BN254: 12 x 4 u64).
 * These are Miller values times subfield factors (openzl_amd/csrc/zl_pairing_dev.hip): only their final exponentiation is defined. */
int zl_test_miller_dev(zl_ctx* ctx, zl_curve_t curve, size_t n, const uint64_t* ps_xy, const uint64_t* qs_xy, uint64_t* out);
/* prod_i e(k_i P_i, Q_i) through the production driver of zl_pairing_product and zl_groth16_verify_batch (device Miller loops with the 128-bit scalars k_i
 * applied inside them, honouring ZL_TUNE_PAIR_GROUPS / ZL_TUNE_PAIR_SET) and the host Engine::final_exp.  scalars128: n x 2 u64 little-endian, NULL = none.
 * ZL_ENOTCURVE for a zero Miller product. */
int zl_test_pairing_product_scaled(zl_ctx* ctx, zl_curve_t curve, size_t n, const uint64_t* ps_xy, const uint64_t* qs_xy, const uint64_t* scalars128,
                                   uint64_t* out12);
/* The host Engine::final_exp of 12 canonical coefficients (in12 -> out12); ZL_ENOTCURVE for a zero input. */
int zl_test_final_exp(zl_curve_t curve, const uint64_t* in12, uint64_t* out12);
/* The device final exponentiation (k_pd_fexp of openzl_amd/csrc/zl_pairing_dev.hip) of `count` values, canonical coefficients in and out as
 * zl_test_final_exp takes them (count x 12 Fq); singular (optional, count bytes): 1 for a zero input, whose result is zero.  ZL_TUNE_FEXP_CHUNK values per launch. */
int zl_test_final_exp_dev(zl_ctx* ctx, zl_curve_t curve, size_t count, const uint64_t* in, uint64_t* out, uint8_t* singular);
/* The inverse in Fq12 by the norm chain of openzl_amd/csrc/zl_fq12_inv.h, run on the host (the kernel takes the same steps, one coefficient per lane): 12
 * canonical coefficients in and out; *singular = 1 and an all-zero result for a zero input.  zl_test_fq12_zeta: the chain's cube root of unity in Fq, canonical. */
int zl_test_fq12_inverse(zl_curve_t curve, const uint64_t* in12, uint64_t* out12, uint8_t* singular);
int zl_test_fq12_zeta(zl_curve_t curve, uint64_t* out);
/* zl_groth16_verify_batch's random linear combination computed entirely on the host (lock-step Engine::multi_pairing, host scalar multiplications), against
 * a verifying key given as points: alpha_g1 (x||y), beta_g2 / gamma_g2 / delta_g2 (x.c0||x.c1||y.c0||y.c1), gamma_abc (n_public + 1 G1 points).  Same rho
 * derivation, rules and outputs as zl_groth16_verify_batch; public_inputs canonical (each < r; otherwise ZL_EINVAL, nothing computed, outputs untouched). */
int zl_test_verify_batch_host(zl_curve_t curve, const uint64_t* alpha_g1, const uint64_t* beta_g2, const uint64_t* gamma_g2, const uint64_t* delta_g2,
                              const uint64_t* gamma_abc, size_t n_public, const zl_g16_proof* proofs, const uint64_t* public_inputs, size_t count,
                              const uint64_t* seed, int* ok, uint8_t* ok_each);

/* The NTT driver's choices, for the tests that must reach every one of them (openzl_amd/csrc/zl_ntt.hip).
 *   zl_test_ntt_plan: the pass plan of a 2^log_n-point transform (log_n <= 32): *P passes of sizes[0..P-1] bits, unused sizes 0.  Host only, no ctx.
 *   zl_test_ntt_fit_beside(ctx, on): sets the ctx's ntt_fit_beside (the passes' 96-register instantiations, otherwise used only by a whole Groth16 proof's
 *   witness map) and returns the previous value; ZL_EINVAL for a null ctx. */
int zl_test_ntt_plan(unsigned log_n, unsigned* P, unsigned sizes[4]);
int zl_test_ntt_fit_beside(zl_ctx* ctx, int on);

/* The scalar split in front of a group's plain MSM (openzl_amd/csrc/zl_msm_endo.h), launched alone: GLV halves on G1, GLS quarters on G2.
 * scalars: n x 4 u64 words (n < 2^24).  out_records: *endo_k x n records of 8 u32 words -- record j n + i = part j of scalar i: magnitude in the low words,
 * sign in bit 31 of word 7 -- followed by ONE more word, the kernel's `bad` flags (bit 0: a scalar with bits at or above the group's scalar width; bit 1: a part
 * at or above 2^*part_bits, which cannot happen); the caller provides 4 n x 8 + 1 words.  *endo_k = parts per scalar (2 / 4), *part_bits = their width (what
 * the MSM plans its windows over).  ZL_EINVAL for a null ctx, n = 0, or a curve / group without a split.
 * zl_test_endo_split_inf additionally takes the per-base infinity flags of the MSM (n bytes, 1 = the base is the point at infinity: its scalar gives zero
 * records; NULL = none). */
int zl_test_endo_split(zl_ctx* ctx, zl_curve_t curve, zl_group_t group, const uint64_t* scalars, size_t n, uint32_t* out_records, int* endo_k, int* part_bits);
int zl_test_endo_split_inf(zl_ctx* ctx, zl_curve_t curve, zl_group_t group, const uint64_t* scalars, const uint8_t* inf, size_t n, uint32_t* out_records, int* endo_k,
                           int* part_bits);

/* The MSM planner's choices, for the tests that must reach every launch form at small sizes (openzl_amd/csrc/zl_msm_job.h, zl_msm.hip).
 * zl_test_msm_plan runs MsmJob::plan alone for a single MSM over points [first, first + n) of the handle -- under the ctx's forced window
 * (zl_ctx_set_msm_window) and the ZL_TUNE_* environment of the moment, exactly as the next zl_msm call would -- and reports the plan: no launch, no device
 * allocation.  The predicates are the members the launch code itself asks (acc_quad, by_cuts, ...), not a copy of their arithmetic.
 *   c, W, SETS, NB: window bits, windows, bucket sets, buckets of all sets; sc_bits: width of what is recoded (the scalar, or a part of its split)
 *   glv, endo_k: the job runs on endo_k parts per scalar (1: plain scalars);  wide: three-level sort;  pre: table of a precomputed handle
 *   chunk, nchunks, big_span: entries per accumulation chunk, chunks, and the cut count above which a bucket leaves the serial fold for the big list
 *   red_g0, red_levels, spread_t: level-0 block length of the bucket reduction, tree levels, and the bits of a spread top window (-1: not spread)
 *   nslices, per_slice, fsl, Gn: sort slices, scalars per slice, level-2 slices (wide sort), sort groups
 *   sort_lds: the LDS counting sort (else wide, or global atomics when !wide);  lds_prefix_small, lds_ranges: its one-block prefix and its scatter ranges (0 otherwise)
 *   fine_cap, fine_threads: staged entries and threads per block of the wide sort's last level (0 unless wide)
 *   acc_quad: four (G2: eight) lanes per chunk in the accumulation, else one lane (G2: a lane pair)
 *   tail_quad_max: tail launches of at most this many lanes run four (eight) lanes per operation;  by_cuts: merge by chunk boundaries, else per bucket
 *   may_big, may_giant: the big / giant bucket kernels are launched
 * ZL_EINVAL for a null ctx or out, ZL_EHANDLE for an unknown handle, otherwise the planner's own code.
 * zl_test_msm_batch_form: how zl_msm_batch_partial_dev / the job driver runs `count` >= 2 jobs, the biggest of `biggest` points: *side = side-by-side lanes (else the
 * three-stream pipeline over three buffer sets), *lanes = buffer sets in rotation, *phased = phase-major issue.  Host only. */
typedef struct zl_test_msm_plan_s {
    int32_t c, W, SETS, NB, sc_bits, glv, endo_k, wide, pre, chunk, nchunks, big_span, red_g0, red_levels, spread_t, nslices, per_slice, fsl, Gn;
    int32_t sort_lds, lds_prefix_small, lds_ranges, fine_cap, fine_threads, acc_quad, tail_quad_max, by_cuts, may_big, may_giant;
} zl_test_msm_plan_t;
int zl_test_msm_plan(zl_ctx* ctx, uint64_t bases, size_t first, size_t n, zl_test_msm_plan_t* out);
int zl_test_msm_batch_form(size_t count, uint64_t biggest, int* side, int* lanes, int* phased);
/* The exact-cover window plan of split BLS12-381 G1 scalars (openzl_amd/csrc/zl_msm_cover_plan.h: widths 22, 21, 21, 21, 21, 22 over 15 sets of 2^19 buckets, the
 * split inside the recoder), which the planner takes by itself only from 2^24 points on.  mode 1: every following plain BLS12-381 G1 MSM of this ctx (no table, no
 * forced window, ZL_NO_GLV unset) runs on it whatever its size -- the same kernels and set layout as at 2^24; mode -1: none does; mode 0: the planner decides.
 * *old_mode (optional) receives the previous mode.  zl_test_msm_plan reports such a plan as glv = 1, c = 20, W = 6, SETS = 15.  ZL_EINVAL for a null ctx or
 * another mode. */
int zl_test_msm_exact_cover(zl_ctx* ctx, int mode, int* old_mode);

/* The point decoders behind zl_points_from_bytes_batch (openzl_amd/csrc/zl_decode.h: lane-uniform square roots, sign rule, multiplication by r), compiled
 * for the HOST: arguments, outputs and statuses as zl_points_from_bytes_batch, no ctx.  The device kernels run the same templates. */
int zl_test_decode_points_host(zl_curve_t curve, zl_group_t group, const uint8_t* in, size_t count, uint64_t* out_xy, uint8_t* out_inf, int32_t* status);
/* fq2_sqrt of that header on n arbitrary Fq2 values (in: n x (c0 || c1) canonical u64 words), on the device when a ctx is given and on the host otherwise.
 * ok[i] = 1 iff value i is a square; out: n roots in the same layout (root^2 == value; either root may come back), all-zero words where ok[i] = 0. */
int zl_test_fq2_sqrt(zl_ctx* ctx, zl_curve_t curve, const uint64_t* in, size_t n, uint64_t* out, uint8_t* ok);

#ifdef __cplusplus
}
#endif
#endif
