// zl_msm_job.h -- one MSM as a plan over device buffers: window choice, buffer layout, and the launch sequences of its three phases
// (sort | accumulate | tail) plus the host Horner.  The drivers in zl_msm.hip run one job, or pipeline several on three streams.
#pragma once
#include <chrono>
#include <stdlib.h>
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
#include "zl_ctx.h"
#include "zl_pool.h"
#include "zl_msm_sort.h"
#include "zl_msm_endo.h"
#include "zl_msm_accumulate.h"
#include "zl_msm_reduce.h"

// BN254 G2 (MsmJob::plan): an MSM takes the four-dimensional split below 2^END points, except in the hole [2^LO, 2^HI), where it keeps its plain windows.  Constants of the
// product, chosen from profiles/bn254_g2_gls_ab.log; only the "open" side of that A/B (tools/ab/bn254_g2_gls_ab.sh) is built with others (0 / 0 / 32: every size up to
// ZL_TUNE_GLV_MAX_LOG splits).
#ifndef ZL_GLS_HOLE_LO_LOG
#define ZL_GLS_HOLE_LO_LOG 11
#define ZL_GLS_HOLE_HI_LOG 17
#define ZL_GLS_END_LOG 19
#endif
static_assert(ZL_GLS_HOLE_LO_LOG >= 0 && ZL_GLS_HOLE_LO_LOG <= ZL_GLS_HOLE_HI_LOG && ZL_GLS_HOLE_HI_LOG <= ZL_GLS_END_LOG && ZL_GLS_END_LOG <= 32, "split below 2^END outside [2^LO, 2^HI)");

// ------------------------------------------------------------------------------------------------ host driver
// developer tuning knobs (profiling sweeps only; unset in production): ZL_TUNE_CHUNK, ZL_TUNE_SEG, ZL_TUNE_FS, ZL_TUNE_RANGES (zl_tune, zl_ctx.h)
static int zl_pick_window(size_t n, int sc_bits, bool wide16 = false /* c = 16 also runs the three-level sort (GLV jobs) */) {
    // cost in accumulated entries: n per window (+10 % for c <= 16: the one-level LDS counting sort streams every window's digits once per
    // bucket range and is the slower sort at large n) + ~4.5 per bucket (merge of cut buckets, level-0 running sums, tree).  Fitted on
    // single-call times at 2^20 .. 2^24, both curves (profiles/r02_msm_sweep_plain.log, r02_msm_sweep_bn254.log), refitted in round 6 (below).  c = 17..20 run the three-level sort over W bucket sets (<= 255 sort groups).
    // (Round 6: 5.7 -> 5.2 with the merge by chunk boundaries, then 4.5: pipelined sweeps of every window at 2^21 .. 2^23 (profiles/r06_window_sweep_2_21_23.log) have 18 ahead of 17 at
    // 2^22 by 1.7 % and 19 ahead of 18 at 2^23 by 4 % -- c = 18 is 15 windows with a nearly empty top one, c = 19 is 14 -- and one constant below 4.6 fits all of 2^20: 16, 2^21: 17, 2^22: 18,
    // 2^23: 19, 2^24: 20.)
    // Split scalars (sc_bits 127 / 64) keep 5.2: at 4.5 BN254's 2^18 moves to c = 16, which is faster alone and 7 % slower inside a proof (zl_pick_window_half below).
    const double per_bucket = (double)zl_tune("ZL_TUNE_BUCKET_COST_X10", sc_bits > 200 ? 45 : 52) / 10.0;
    double best = 1e300;
    int best_c = 2;
    for (int c = 2; c <= 20; c++) {
        int W = (sc_bits + 1 + c - 1) / c;
        if (c > 16 && (((uint64_t)W << (c - 1)) >> 15) > 255) continue;
        const bool lds_sort = c < 16 || (c == 16 && !wide16);
        double cost = (double)n * W * (lds_sort ? 1.10 : 1.0) + per_bucket * W * (double)(1u << (c - 1));
        if (cost < best) { best = cost; best_c = c; }
    }
    return best_c;
}

// The 127-bit half-scalars of an endomorphism split on G1 (2 n entries per window, half the windows): the cost model above is fitted on machine-filling sizes and misses
// what decides a latency-bound MSM (which sort runs, chunk length, four-lane or one-lane kernels): at 2^18 points it picks c = 15 where c = 16 is 13 % faster, at 2^13 / 2^14
// c = 10 / 11 where 11 / 12 are 8-10 % faster.  Measured best window by size, entries only where the gain is clear and survives inside a proof (profiles/r06_glv_window_sweep.log: every c in 9 .. 17
// at 2^11 .. 2^19 points); 0 = outside the table, the model decides.
static int zl_pick_window_half(size_t n_points) {
    if (n_points < 2) return 0;
    int lg = 63 - __builtin_clzll((unsigned long long)n_points);
    if ((double)n_points >= 1.4142 * (double)((size_t)1 << lg)) lg++;  // nearest power of two
    static const signed char best[9] = {9, 0, 11, 12, 0, 0, 0, 16, 0};  // 2^11 .. 2^19 points; 0 = the model (ties as single calls; c = 12 at 2^16 made a 57 000-constraint proof 8 % slower)
    return lg >= 11 && lg <= 19 ? best[lg - 11] : 0;
}
// ... and the 64-bit quarter-scalars of the G2 split (4 n entries per window): the model's 11 at 2^13 / 2^14 where 12 / 13 are 8-10 % faster, 17 at 2^18 where 14 is 5 % faster
// (profiles/r06_half_table_ab.log, "G2 window sweep": every c in 8 .. 16 at 2^10 .. 2^18 points).  Measured on BLS12-381; BN254's quarters are 64 bits too
// (BN254_GLS::QUARTER_BITS) and run the same kernels on 10 limbs instead of 14, so they take the same table: an assumption, neither swept nor measured on BN254.
static int zl_pick_window_quarter(size_t n_points) {
    if (n_points < 2) return 0;
    int lg = 63 - __builtin_clzll((unsigned long long)n_points);
    if ((double)n_points >= 1.4142 * (double)((size_t)1 << lg)) lg++;
    static const signed char best[9] = {9, 0, 11, 12, 13, 13, 13, 13, 14};  // 2^10 .. 2^18 points (0: not measured, the model)
    return lg >= 10 && lg <= 18 ? best[lg - 10] : 0;
}

// The exact-cover plan of split BLS12-381 G1 scalars (zl_msm_cover_plan.h): widths 22, 21, 21, 21, 21, 22 over sets of 2^19 buckets -- what the device sees at
// c = 20, with 15 sets for 13 and 12 entries per point for 13.  It trades one mixed addition per point for ~0.9 M more live buckets, the split and the sort of
// 2 n records, which pays only where n entries outweigh them: from 2^ZL_COVER_MIN_LOG points on (profiles/exact_cover_ab.log).
#ifndef ZL_COVER_MIN_LOG
#define ZL_COVER_MIN_LOG 24
#endif
#define ZL_COVER_SET_LOG 19
static const uint32_t ZL_COVER_WIDTHS[6] = {22, 21, 21, 21, 21, 22};
static bool zl_pick_cover(size_t n_points) { return (uint64_t)n_points >= (1ull << ZL_COVER_MIN_LOG); }

static int zl_pick_window_precomp(size_t n, int sc_bits) {
    // merged windows: n*W mixed adds + ONE bucket set of 2^(c-1) buckets (merge + reduce ~6 add-equivalents per bucket)
    // measured at 2^20: c = 16 and c = 20 tie for a single call (4.9 ms), 17..19 are slower (half-filled staging blocks), and inside a
    // pipeline (Groth16's five MSMs) c = 20 wins clearly: fewer additions, and the larger sort / tail are hidden
    if (n < (size_t)700000) return 16;
    if (n < ((size_t)1 << 21)) return 20;
    double best = 1e300;
    int best_c = 16;
    for (int c = 20; c <= 23; c++) {
        int W = (sc_bits + 1 + c - 1) / c;
        double cost = (double)n * W + 6.0 * (double)(1u << (c - 1));
        if (cost < best) { best = cost; best_c = c; }
    }
    return best_c;
}

// One MSM as three phases that only communicate through device buffers, so that consecutive MSMs can be pipelined on three streams
// (sort of MSM i+2 | bucket accumulation of MSM i+1 | merge / reduction tail of MSM i): plan() sizes everything, alloc() binds one of
// three buffer sets, sort() builds the bucket-sorted entry list, accumulate() is the dominant kernel, tail() leaves SETS window sums
// (+ the sum of the scalar-1 bases) in host memory, finish() does the host Horner.
// Byte layout of a planned job's two sort temporaries (slot A, slot B).  plan_as fills it and is the only place this arithmetic exists: alloc
// sizes and binds the slots from it, the sort functions add the offsets to the bound pointers.
struct MsmSortLayout {
    size_t a_bytes = 0, b_bytes = 0;  // what the job needs of slot A / slot B (0: nothing -- the global-atomics sort)
    uint32_t nslices = 0, per_slice = 0;
    // three-level sort.  A: lo16 | hi8 | part_lo | part_idx | partition counters (P counts, P + 1 offsets, block sums); B: lo2 | idx2 | counters2 (likewise over P2)
    size_t hi8 = 0, part_lo = 0, part_idx = 0, pcounts = 0, idx2 = 0, counts2 = 0;
    uint32_t P = 0, pscan_blocks = 0, fsl = 0, P2 = 0, p2scan_blocks = 0;
    // LDS sort.  A: digits | per-slice bucket counts
    size_t slice_counts = 0;
    size_t vs = 0;  // GLV: the half-scalars, behind A's temporaries
};
template <class G>
struct MsmJob {
    using F = typename G::F;
    using X = XYZZ<F>;
    // plan
    bool pre = false;
    int c = 0, W = 0;
    int spread_t = -1;  // >= 0: the top window's entries are spread over its bucket set, weights = low spread_t bits + 1
    bool wide = false;  // three-level sort over (window, bucket) ids of up to 23 bits: table mode, or plain windows wider than 16 bits
    bool glv = false;   // the job runs on 2 n_real half-scalars of 127 bits over the points P_i and phi(P_i) (k_glv_split / k_glv_phi)
    bool cover = false;  // a glv job on an exact-cover plan (cv): W digit rows of unequal widths over SETS uniform sets; the recoder splits, no half-scalar records
    zl_cover_plan cv;
    bool phi_cached = false;  // d_phi is the handle's own copy (zl_bases::d_endo)
    bool phi_owner = false;  // this job computes the phi image of its bases in its sort phase (else it borrows d_phi from an earlier job of the call)
    int sc_bits = 0, endo_k = 1;  // endo_k: half-scalars per scalar (2: GLV on G1, 4: GLS on G2)
    zl_slot phi_slot = ZL_SLOT_PHI_ONE_KEY;
    MsmSortLayout lay;
    unsigned char *d_sort_a = nullptr, *d_sort_b = nullptr;  // the sort temporaries (ZL_SLOT_SORT_A / _B: shared by the jobs of a pipelined batch; the set's own pair when small jobs run side by side)
    size_t n_real = 0;
    uint32_t* d_vs = nullptr;            // the half-scalars (inside the sort temporaries)
    const Affine<F>* d_phi = nullptr;    // phi(P_i), i < n_real
    uint32_t H = 0, SETS = 0, NB = 0, ZL_CHUNK = 0, nchunks = 0, scan_blocks = 0, max_big = 0, max_giant = 0, Gn = 0, big_span = ZL_BIG_SPAN;
    uint32_t red_g0 = 0, red_lg0 = 0, red_blocks = 0, red_levels = 0;  // bucket reduction: block length of level 0, blocks per set, tree levels
    uint32_t roots_per_set = 0;                                         // channels of a set's root node: T, A, S_0 .. S_(levels-1)
    uint64_t maxE = 0;
    size_t n = 0, first = 0;
    const zl_bases* bsp = nullptr;
    // buffers
    uint32_t *d_counts = nullptr, *d_offsets = nullptr, *d_cursor = nullptr, *d_entries = nullptr, *d_block_sums = nullptr, *d_big_list = nullptr,
             *d_big_count = nullptr, *d_ones_count = nullptr, *d_giant_count = nullptr, *d_giant_list = nullptr, *d_ones_list = nullptr,
             *d_bigsg_items = nullptr, *d_bad_scalar = nullptr, *d_chunk_head = nullptr;
    unsigned long long* d_bigsg_head = nullptr;
    X *d_buckets = nullptr, *d_partials = nullptr, *d_segs = nullptr, *d_stage1 = nullptr, *d_sets = nullptr, *d_ones_parts = nullptr, *d_giant_tmp = nullptr;
    const Affine<F>* d_bases = nullptr;
    const uint8_t* d_inf = nullptr;  // per-base infinity flags of the range (null: the handle has no point at infinity)
    const uint32_t* sc = nullptr;
    // host results (pinned when pipelined)
    X* hw = nullptr;
    uint32_t* hE = nullptr;  // [0] = entries accumulated, [1] = non-canonical-scalar flag
    std::vector<X> hw_own;
    // result buffer (pinned when pipelined): SETS * roots_per_set root channels, the scalar-1 sum, then the two status words k_msm_ones leaves behind it
    void set_host_buffer(X* buf) {
        hw = buf;
        hE = reinterpret_cast<uint32_t*>(buf + (size_t)SETS * roots_per_set + 1);
    }

    // phi_slot_: scratch slot for the endomorphism image of the bases when this job computes it (GLV)
    int plan(zl_ctx* ctx, const zl_bases& bs, size_t first_, const void* d_scalars, size_t n_, zl_slot phi_slot_) {
        static const bool no_glv = getenv("ZL_NO_GLV") != nullptr;  // developer A/B switch
        bool try_glv = false;
        // Measured (round 3, profiles/r03_glv_ab.log): halving the bucket sets wins where the merge / reduction tails and the host Horner dominate
        // (2^16: 1.07 -> 1.00 ms, 2^18: 1.67 -> 1.63 ms, Groth16 k = 64: 3.8 -> 3.6 ms); from 2^20 on the split, the phi image of the bases
        // (read + write of every point) and the three-level sort of 2 n records cost what the tail saves (2^20: 3.73 = 3.73 ms; 2^24 single
        // call 39.2 -> 39.7 ms, pipelined 36.7 = 36.7), so large inputs keep the plain 255-bit windows.
        // (That was at EQUAL entry counts, one width for every window.  From 2^24 points on BLS12-381 G1 splits again, on widths that cover the half-scalar exactly: below.)
        static const size_t glv_max = (size_t)1 << zl_tune("ZL_TUNE_GLV_MAX_LOG", 19);
        if constexpr (G::GLV) try_glv = bs.precomp_c == 0 && !no_glv && n_ >= 1 && n_ <= glv_max && (uint64_t)n_ * G::ENDO_K < (1ull << 31);
        // BN254 G1 (round 6: two-dimensional split, k_glv_split_lattice): its host Horner is cheap (254 doublings at 0.3 us) against the split's extra device work (2 n
        // sort records, one more kernel), so between 2^13 and 2^17 points the plain windows are 3-4 % faster as a single call and 8 % pipelined -- BASELINE config 1's size
        // among them -- while 2^10 (-15 %), 2^17 (-14 %) and 2^19 (-9 %) gain (profiles/r06_small_knobs2.log, r06_bn_glv_ab.log).  BLS12-381 never loses (same logs).
        if constexpr (G::GLV && G::ENDO_K == 2) {
            if constexpr (G::GLVP::LATTICE) {
                if (n_ >= ((size_t)1 << 13) && n_ < ((size_t)1 << 17)) try_glv = false;
            }
        }
        // BN254 G2 (four-dimensional split, k_gls_split_lattice; interleaved A/B against the commit before it at 2^8 .. 2^20 points, three runs a side, run-to-run spread
        // 0.2-7 %: profiles/bn254_g2_gls_ab.log).  A single call gains at every size up to 2^18 (2^8: 0.55 -> 0.37 ms, 2^10: 0.59 -> 0.34, 2^14: 0.77 -> 0.62, 2^17: 1.79 -> 1.53,
        // 2^18: 2.34 -> 2.16), ties at 2^19 and loses 6 % at 2^20 (5.62 -> 5.96).  Pipelined (batches of 8, per MSM) it gains at 2^8 - 2^10 (2^10: 0.185 -> 0.153) and at 2^17 / 2^18
        // (1.32 -> 1.01, 1.90 -> 1.59), but LOSES at 2^11 (0.196 -> 0.222) and 2^13 (0.245 -> 0.322) and ties at 2^12 and 2^14 - 2^16, where the device chain of 4 n records costs what the
        // shorter host Horner saves once the Horner is hidden behind the next job; 2^19: -2 %, 2^20: -8 %.  The gate is by size alone, so it keeps the sizes that win both ways:
        // n < 2^11 and 2^17 <= n < 2^19.  Measured: the powers of two; the bounds between 2^10 and 2^11, 2^16 and 2^17, 2^18 and 2^19 are put at the first measured size that
        // does not win.  (The single-call gains at 2^11 - 2^16, 6-34 %, are left for a gate that knows whether the job is pipelined.)
        if constexpr (G::GLV && G::ENDO_K == 4) {
            if constexpr (G::GLVP::LATTICE) {
                if (((uint64_t)n_ >= (1ull << ZL_GLS_HOLE_LO_LOG) && (uint64_t)n_ < (1ull << ZL_GLS_HOLE_HI_LOG)) || (uint64_t)n_ >= (1ull << ZL_GLS_END_LOG)) try_glv = false;
            }
        }
        // BLS12-381 G1 from 2^ZL_COVER_MIN_LOG points on: the split with an exact-cover plan (zl_pick_cover above).  A forced window (zl_ctx_set_msm_window) keeps its
        // uniform windows; ctx->msm_cover is the tests' switch (zl_test_msm_exact_cover: > 0 the plan at any size, < 0 never).
        if constexpr (G::GLV && G::ENDO_K == 2) {
            if constexpr (!G::GLVP::LATTICE) {
                const bool want = ctx->msm_cover > 0 || (ctx->msm_cover == 0 && zl_pick_cover(n_));
                if (want && bs.precomp_c == 0 && !no_glv && ctx->msm_c <= 0 && n_ >= 1 && (uint64_t)n_ * 2 * ZL_CV_MAX_WINDOWS < (1ull << 32)) {
                    int rc = plan_as(ctx, bs, first_, d_scalars, n_, true, true);
                    if (!rc && cover) {
                        phi_slot = phi_slot_;
                        phi_owner = true;
                        return rc;
                    }
                }
            }
        }
        int rc = plan_as(ctx, bs, first_, d_scalars, n_, try_glv);
        // (c <= 3: the top window of a 127-bit half-scalar can reach magnitude H + carry; not worth a special case)
        if (!rc && glv && c <= 3) rc = plan_as(ctx, bs, first_, d_scalars, n_, false);
        // the global-atomics sort (forced plain c >= 21 beyond 255 sort groups) does not take half-scalars: plan again without them
        if (!rc && glv && !wide && c > 16) rc = plan_as(ctx, bs, first_, d_scalars, n_, false);
        phi_slot = phi_slot_;
        phi_owner = glv;
        return rc;
    }
    int plan_as(zl_ctx* ctx, const zl_bases& bs, size_t first_, const void* d_scalars, size_t n_, bool glv_, bool cover_ = false) {
        glv = glv_;
        cover = false;
        if constexpr (G::GLV && G::ENDO_K == 2) {
            if constexpr (!G::GLVP::LATTICE) {
                if (cover_ && glv_ && bs.precomp_c == 0) {
                    using P = typename G::GLVP;
                    uint32_t lam[4], bar[8], rm[8];
                    for (int k = 0; k < 4; k++) lam[k] = P::lambda(k);
                    for (int k = 0; k < 8; k++) { bar[k] = P::barrett(k); rm[k] = P::rmod(k); }
                    // the obligations of the plan, from the split's constants: a plan that does not hold is not used
                    cover = zl_cover_make(cv, ZL_COVER_WIDTHS, 6, ZL_COVER_SET_LOG, lam, bar, rm) == ZL_CV_OK;
                }
            }
        }
        n_real = n_;
        endo_k = glv ? (int)G::ENDO_K : 1;
        n = (size_t)endo_k * n_;
        sc_bits = !glv ? (int)G::SC_BITS : MsmJobPartBits<G>::value;  // (zl_msm_endo.h)
        first = first_;
        bsp = &bs;
        pre = bs.precomp_c > 0;  // table of 2^(c w) P_i present: all windows share one bucket set
        c = pre ? bs.precomp_c : (ctx->msm_c > 0 ? ctx->msm_c : zl_pick_window(n, sc_bits, glv && G::ENDO_K != 2));
        if (!pre && ctx->msm_c <= 0 && glv) {
            int h = 0;
            if constexpr (G::ENDO_K == 2) {
                // (BN254: c = 16 at 2^18 is 11 % faster as a single call and 7 % SLOWER inside a 240 000-constraint proof, where four such MSMs and the witness map share
                // the machine -- the table is BLS12-381's, profiles/r06_tables_mid_ab.log)
                if (!G::GLVP::LATTICE) h = zl_pick_window_half(n_);
            } else {
                h = zl_pick_window_quarter(n_);
            }
            if (h) c = h;
        }
        if (c < 2) c = 2;
        if (c > 24) c = 24;
        W = (sc_bits + 1 + c - 1) / c;
        if (cover) {  // W digit rows over SETS uniform sets of 2^set_log buckets: the device's view is that of c = set_log + 1
            c = (int)cv.set_log + 1;
            W = (int)cv.windows;
        }
        H = 1u << (c - 1);
        SETS = pre ? 1u : (cover ? cv.nsets : (uint32_t)W);  // bucket sets
        const uint64_t NB64 = (uint64_t)SETS * H;
        maxE = (uint64_t)n * W;
        if (n >= (1ull << 31) || maxE >= (1ull << 32) || NB64 >= (1ull << 31)) return ZL_EINVAL;
        if (pre && (uint64_t)W * bs.n >= (1ull << 31)) return ZL_EINVAL;
        NB = (uint32_t)NB64;
        Gn = NB >> 15;  // sort groups of 32768 (window, bucket) ids; the group id travels in a byte, 0xFF = zero digit
        if (pre && (c < 16 || Gn < 1 || Gn > 255)) return ZL_EINVAL;
        // plain windows beyond that (c >= 21) fall back to the global-atomics sort.  GLS quarter-scalars (G2) at c = 16 take the wide sort too: their
        // narrow top window is spread over the bucket set, and a spread bucket index of all ones with the sign set would be the LDS sort's 0xFFFF =
        // "zero digit" (GLV half-scalars on G1 have a full top window and a tie rule that keeps the code free: k_msm_recode)
        wide = pre || ((c > 16 || (glv && c == 16 && G::ENDO_K != 2)) && Gn >= 1 && Gn <= 255);
        // chunk length: 64 entries per lane once there are enough entries to fill the chip (~2^18 lanes), shorter below
        // (128 once there are >= 2^20 lanes of that length: half as many cut buckets to merge; 32.8 -> 32.2 ms per pipelined 2^24 MSM)
        ZL_CHUNK = (maxE >> 7) >= (1u << 20) ? 128u : (uint32_t)ZL_CHUNK_MAX;
        while (ZL_CHUNK > 8 && maxE / ZL_CHUNK < (1u << 18)) ZL_CHUNK >>= 1;
        // ... but never so short that an average bucket is cut into more than ~4 chunks: beyond ZL_BIG_SPAN_SMALL = 8 chunks a bucket leaves the lane-serial fold of
        // k_msm_merge for one WORKGROUP per bucket (k_msm_merge_big), which is meant for the few heavy buckets of a skewed input, not for all of them.  Round 6 found
        // the case in a sweep: a 2^14-point G2 MSM (GLS: 65 536 quarter-scalars, c = 11, 64 entries per bucket, 8-entry chunks) spent 3 of its 3.5 ms there --
        // slower than the 2^16-point MSM (1.4 ms).
        // (Half-scalars of an endomorphism split fill only part of their top window's range -- |k_i| <= 0.67 * 2^127 on BLS12-381, 0.43 * 2^127 on BN254 -- so that
        // window's buckets are 1.5-2.3x as dense as the average: counted double.  A 2^14-point G1 MSM, 32 entries per bucket on average and 8-entry chunks, sent a
        // handful of its top window's buckets to k_msm_merge_big: 82 us of a 0.56-ms device chain, profiles/r06_timeline_msm_2_14_glv.txt.)
        // (Quarter-scalars of the G2 splits: BLS12-381's base-|z| digits are uniform below |z| = 0.82 * 2^64, a top window 1.2x as dense as the average: counted once.
        // BN254's lattice quarters are sums of four roundings and crowd towards 0 far below their proved bound (FILL_PCT): of random scalars the busiest 1/32 of
        // [0, 2^64) holds PEAK_PCT = 370 % of an even share (tools/gen_bn254_gls.py), so a full top window's low buckets are 3-3.7x as dense as the average: counted
        // double like the halves, which keeps such a bucket at 3.7 / 2 * 4 = 7.4 chunks, within k_msm_merge's ZL_BIG_SPAN_SMALL.)
        uint32_t dense = glv && G::ENDO_K == 2 ? 2u : 1u;
        if constexpr (G::GLV && G::ENDO_K == 4) {
            if constexpr (G::GLVP::LATTICE) {
                static_assert(G::GLVP::PEAK_PCT <= 400, "the top window's busiest buckets are more than 4x the average: a factor of 2 no longer keeps them below 8 chunks");
                if (glv && G::GLVP::PEAK_PCT > 200) dense = 2u;
            }
        }
        while (ZL_CHUNK < (uint32_t)ZL_CHUNK_MAX && dense * (maxE / std::max<uint64_t>(1, (uint64_t)SETS * H)) > (uint64_t)4 * ZL_CHUNK) ZL_CHUNK <<= 1;
        ZL_CHUNK = (uint32_t)std::max(8, zl_tune("ZL_TUNE_CHUNK", (int)ZL_CHUNK));
        nchunks = (uint32_t)((maxE + ZL_CHUNK - 1) / ZL_CHUNK);
        // bucket reduction (k_msm_reduce_level0 + k_msm_reduce_tree): blocks of 8 buckets (4 / 2 for smaller inputs: more lanes, shorter chains)
        {
            // measured (gpurun sweep of ZL_TUNE_SEG, round 3): 2 up to 2^16 points, 4 at 2^18 - 2^20, 8 from 2^22 on
            uint32_t g0 = NB >= (1u << 20) ? 8u : (NB >= (1u << 17) ? 4u : 2u);
            g0 = (uint32_t)std::max(2, zl_tune("ZL_TUNE_SEG", (int)g0));
            while (g0 & (g0 - 1)) g0 &= g0 - 1;
            if (g0 > H) g0 = H;
            // plain wide windows: spread the narrow top window over its whole bucket set (k_msm_recode_wide); the weight then lives in the
            // low spread_t bits of the bucket index: all of level 0's bits must be on one side of that boundary (a very narrow top
            // window, 0 < spread_t < log2 g0, shortens the level-0 blocks to 2^spread_t)
            spread_t = -1;
            if ((wide || c <= 16) && !pre && !cover) {  // (an exact-cover plan has no narrow top window; the global-atomics sort of plain c >= 21 keeps its crowded top window)
                const int top_bits = sc_bits + 1 - (W - 1) * c;  // bits of the top window incl. the carry: magnitudes <= 2^(top_bits - 1)
                if (top_bits - 1 < c - 1) {
                    spread_t = top_bits - 1;
                    if (spread_t > 0 && (1u << spread_t) < g0) g0 = 1u << spread_t;
                }
            }
            red_g0 = g0;
            red_lg0 = 31 - __builtin_clz(g0);
            red_blocks = H / g0;  // both powers of two
            red_levels = 31 - __builtin_clz(red_blocks);
            roots_per_set = red_levels + 2;
        }
        scan_blocks = (NB + SCAN_BLOCK * SCAN_ITEMS - 1) / (SCAN_BLOCK * SCAN_ITEMS);
        big_span = nchunks <= (1u << 17) ? (uint32_t)ZL_BIG_SPAN_SMALL : (uint32_t)ZL_BIG_SPAN;
        max_big = (uint32_t)(maxE / ((uint64_t)ZL_CHUNK * big_span)) + 1;
        max_giant = (uint32_t)(maxE / ((uint64_t)ZL_CHUNK * ZL_GIANT_SPAN)) + 1;
        // the sort temporaries (every part rounded up to 256 bytes)
        lay = MsmSortLayout{};
        auto up256 = [](size_t b) { return (b + 255) / 256 * 256; };
        const uint32_t max_slices = (uint32_t)((n + 4095) / 4096);
        if (wide) {
            lay.nslices = std::min<uint32_t>(64, max_slices);
            lay.P = Gn * W * lay.nslices;  // partition counters, order (group, window, slice)
            lay.pscan_blocks = (lay.P + SCAN_BLOCK * SCAN_ITEMS - 1) / (SCAN_BLOCK * SCAN_ITEMS);
            const size_t b_lo = up256((size_t)n * W * 2), b_hi = up256((size_t)n * W), b_idx = up256((size_t)n * W * 4);
            lay.hi8 = b_lo;
            lay.part_lo = lay.hi8 + b_hi;
            lay.part_idx = lay.part_lo + b_lo;
            lay.pcounts = lay.part_idx + b_idx;
            lay.a_bytes = lay.pcounts + up256((size_t)(2 * lay.P + lay.pscan_blocks + 8) * 4) + 256;
            // level 2: 128 sub-groups (256 buckets each) per group, counted in fsl slices
            lay.fsl = 16;
            while (lay.fsl * Gn < 2048 && lay.fsl < 128) lay.fsl *= 2;
            lay.P2 = Gn * 128 * lay.fsl;
            lay.p2scan_blocks = (lay.P2 + SCAN_BLOCK * SCAN_ITEMS - 1) / (SCAN_BLOCK * SCAN_ITEMS);
            lay.idx2 = b_lo;
            lay.counts2 = lay.idx2 + b_idx;
            lay.b_bytes = lay.counts2 + up256((size_t)(2 * (size_t)lay.P2 + lay.p2scan_blocks + 8) * 4) + 256;
        } else if (c <= 16) {
            lay.nslices = std::max<uint32_t>(1, std::min<uint32_t>((256 + W - 1) / W, max_slices));  // ~256+ blocks of 1024 lanes, one per CU (<= 128 KiB LDS each)
            lay.slice_counts = up256((size_t)n * W * 2);
            lay.a_bytes = (size_t)n * W * 2 + (size_t)lay.nslices * NB * 4 + 256;  // (the trailing 256 covers the rounding of the digits)
        }  // plain c >= 21 (more than 255 sort groups): the global-atomics sort needs no temporaries
        if (lay.nslices) lay.per_slice = (uint32_t)((n + lay.nslices - 1) / lay.nslices);
        if (glv && !cover) {  // (an exact-cover plan splits inside its recoder: no half-scalar records)
            lay.vs = up256(lay.a_bytes);
            lay.a_bytes = lay.vs + up256((size_t)n * 32);
        }
        if (cover && (!wide || Gn != (cv.nsets << (cv.set_log - ZL_CV_GROUP_LOG)) || Gn > 255)) return ZL_EINVAL;  // the recoder's group ids are the sort's (0xFF = zero digit)
        d_bases = pre ? reinterpret_cast<const Affine<F>*>(bs.d_table) : reinterpret_cast<const Affine<F>*>(bs.d_pts) + first;
        d_inf = bs.d_inf ? reinterpret_cast<const uint8_t*>(bs.d_inf) + first : nullptr;
        sc = reinterpret_cast<const uint32_t*>(d_scalars);
        hw_own.assign((size_t)SETS * roots_per_set + 2, X::inf());  // (+ one element of room for the two status words behind the result)
        set_host_buffer(hw_own.data());
        return ZL_OK;
    }
    // ---- the launch forms that follow from the plan: sort(), accumulate() and tail() below ask these members, and so does the plan report of the tests
    // (zl_msm_plan_report, zl_msm.hip), so that a test asserts the branch the launch code takes and not a copy of its arithmetic
    bool sort_is_lds() const { return !wide && c <= 16; }  // else the three-level sort (wide) or, beyond 255 sort groups, global atomics
    bool lds_prefix_small() const { return NB <= 14336 && lay.nslices <= 64; }  // (14 336 buckets: 59.6 KB of LDS for the totals beside the 4 KB of the scan)
    // LDS sort, scatter: one block per (bucket range, window); ranges sized so that W * ranges ~ 256..512 blocks
    uint32_t lds_ranges() const {
        uint32_t ranges = 1;
        while (ranges * W < 256 && (H / (ranges * 2)) >= 64) ranges *= 2;
        return (uint32_t)std::max(1, zl_tune("ZL_TUNE_RANGES", (int)ranges));
    }
    // wide sort, level 3: staged entries per block: at most 144 KiB + 1 KiB of cursors (1 block per CU); sub-groups average n*W/SG entries, so many small
    // sub-groups (plain wide windows) get a smaller stage and two blocks per CU.  A sub-group above the cap goes to k_msm_fine_sort_big's queue.
    uint32_t fine_cap() const {
        const uint32_t SG = Gn * 128;
        const uint32_t cap = (uint32_t)std::min<uint64_t>(36 * 1024, std::max<uint64_t>(4096, (maxE / SG) * 22 / 10));
        return (uint32_t)std::max(1024, zl_tune("ZL_TUNE_FS_CAP", (int)cap));
    }
    uint32_t fine_threads() const { return (uint32_t)zl_tune("ZL_TUNE_FS", 1024); }
    // four lanes per chunk (Fq2 groups: eight) while that is at most ~1.5 waves per SIMD (round 6: 49 152 -> 24 576; at three waves per SIMD the one-lane kernel
    // is faster: 94 against 131 us at 2^14, profiles/r06_small_knobs2.log)
    bool acc_quad() const { return nchunks <= (uint64_t)zl_tune("ZL_TUNE_QUAD_ACC_CHUNKS", 24576); }
    // four lanes per group operation (zl_quad.h; Fq2 groups: eight, zl_fq2pair.h) in every tail launch of at most this many lanes, one lane (Fq2: a lane pair) beyond
    uint32_t tail_quad_max() const { return (uint32_t)zl_tune("ZL_TUNE_QUAD_LANES", 65536); }
    bool by_cuts() const { return NB > tail_quad_max() && nchunks > 1; }  // one lane (pair) per chunk boundary: every surviving lane folds one bucket
    // a bucket cut into more than big_span (ZL_GIANT_SPAN) chunks needs that many chunks to exist: small jobs skip the launches (three of the ~22 of a small MSM's chain)
    bool may_big() const { return nchunks > big_span; }
    bool may_giant() const { return nchunks > (uint32_t)ZL_GIANT_SPAN; }

    // buffer set 0..3 (ZL_MSM_SET, zl_ctx.h).  own_sort: the job's sort runs beside the other sets' sorts, in the set's own temporaries; otherwise in
    // ZL_SLOT_SORT_A / _B, which the jobs of a call share: their sorts run in order on one stream.  Callers bind every job before anything is in
    // flight (a growing zl_scratch_get frees the old block), and again once every slot has reached its largest user.
    int alloc(zl_ctx* ctx, int set, bool own_sort = false) {
        void* p;
        int rc;
        const zl_msm_set_slots& slots = ZL_MSM_SET[set];
        d_sort_a = d_sort_b = nullptr;
        if (lay.a_bytes) {
            if ((rc = zl_scratch_get(ctx, own_sort ? slots.sort_a : ZL_SLOT_SORT_A, lay.a_bytes, &p))) return rc;
            d_sort_a = (unsigned char*)p;
        }
        if (lay.b_bytes) {
            if ((rc = zl_scratch_get(ctx, own_sort ? slots.sort_b : ZL_SLOT_SORT_B, lay.b_bytes, &p))) return rc;
            d_sort_b = (unsigned char*)p;
        }
        // counters (NB+1) | offsets (NB+2: [NB] = total entries, [NB+1] = non-canonical-scalar flag) | cursor (NB+1) | block sums | big list | counts | giant list | scalar-1 list |
        // oversized sub-groups | chunk heads (G1: the bucket every chunk starts in, left by the accumulation for k_msm_merge_cuts; per set like the offsets it indexes)
        const size_t max_bigsg = (size_t)(maxE / 1024) + 2;  // oversized sub-groups hold > cap >= 1024 entries each
        size_t small_words = (size_t)3 * (NB + 1) + 1 + scan_blocks + 1 + max_big + max_giant + 16 + n + 2 * max_bigsg + nchunks;
        if ((rc = zl_scratch_get(ctx, slots.data[0], small_words * 4, &p))) return rc;
        d_counts = (uint32_t*)p;
        d_offsets = d_counts + (NB + 1);
        d_cursor = d_offsets + (NB + 2);
        d_block_sums = d_cursor + (NB + 1);
        d_big_list = d_block_sums + scan_blocks + 1;
        d_big_count = d_big_list + max_big;
        d_ones_count = d_big_count + 1;
        d_giant_count = d_big_count + 2;
        d_bad_scalar = d_big_count + 3;  // zeroed with the counts; set by the recoder for a scalar with bits >= SC_BITS
        d_giant_list = d_big_count + 16;
        d_ones_list = d_giant_list + max_giant;
        d_bigsg_items = d_ones_list + n;
        d_chunk_head = d_bigsg_items + 2 * max_bigsg;
        d_bigsg_head = reinterpret_cast<unsigned long long*>((reinterpret_cast<uintptr_t>(d_big_count + 4) + 7) & ~(uintptr_t)7);  // inside words 4..7
        if ((rc = zl_scratch_get(ctx, slots.data[1], maxE * 4, &p))) return rc;
        d_entries = (uint32_t*)p;
        if ((rc = zl_scratch_get(ctx, slots.data[2], (size_t)NB * sizeof(X), &p))) return rc;
        d_buckets = (X*)p;
        if ((rc = zl_scratch_get(ctx, slots.data[3], (size_t)2 * nchunks * sizeof(X), &p))) return rc;
        d_partials = (X*)p;
        // ping-pong node buffers of the reduction tree: leaves = 2 channels x blocks, level 1 = 3 channels x blocks / 2 (the largest)
        const size_t leaf_elems = (size_t)2 * SETS * red_blocks, lvl1_elems = (size_t)3 * SETS * (red_blocks / 2 + 1);
        const size_t root_elems = (size_t)SETS * roots_per_set;
        // (per set: the tails of consecutive jobs may overlap)
        if ((rc = zl_scratch_get(ctx, slots.tail, (leaf_elems + lvl1_elems + root_elems + 2 + ZL_ONES_BLOCKS + (size_t)max_giant * ZL_GIANT_PARTS) * sizeof(X), &p))) return rc;
        d_segs = (X*)p;                    // tree nodes, even levels (level 0 = leaves)
        d_stage1 = d_segs + leaf_elems;    // tree nodes, odd levels
        d_sets = d_stage1 + lvl1_elems;    // the root channels of every set, then the sum of the scalar-1 bases
        d_ones_parts = d_sets + root_elems + 2;  // (one element of room behind the scalar-1 sum: the two status words k_msm_ones writes there)
        d_giant_tmp = d_ones_parts + ZL_ONES_BLOCKS;
        if (glv) {
            // The images depend on the bases only: kept with the handle (one range per handle; another range of the same handle falls back to
            // the per-call scratch copy below).  k_gls_psi is 50 us of latency in front of the G2 MSM of every small proof, k_glv_phi 12-100 us.
            const size_t endo_bytes = (size_t)(endo_k - 1) * n_real * sizeof(Affine<F>);
            const zl_bases& bs = *bsp;
            std::lock_guard<std::mutex> cache_lk(zl_bases_cache_mutex());  // the handle may be shared by the lanes of a forked ctx
            if (!bs.d_endo && endo_bytes <= ((size_t)zl_tune("ZL_TUNE_ENDO_CACHE_MB", 512) << 20)) {
                void* q = nullptr;
                if (hipMalloc(&q, endo_bytes) == hipSuccess) {
                    if constexpr (G::GLV && G::ENDO_K == 2)
                        hipLaunchKernelGGL((k_glv_phi<G>), dim3((uint32_t)((n_real + 127) / 128)), dim3(128), 0, ctx->stream, d_bases, (uint32_t)n_real, reinterpret_cast<Affine<F>*>(q));
                    else if constexpr (G::GLV && G::ENDO_K == 4)
                        hipLaunchKernelGGL((k_gls_psi<G>), dim3((uint32_t)((n_real + 63) / 64)), dim3(64), 0, ctx->stream, d_bases, (uint32_t)n_real, reinterpret_cast<Affine<F>*>(q));
                    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) { (void)hipFree(q); return ZL_EHIP; }
                    bs.d_endo = q;
                    bs.endo_first = first;
                    bs.endo_n = n_real;
                    bs.endo_k = endo_k;
                } else {
                    (void)hipGetLastError();  // out of memory for the cache: clear HIP's sticky per-thread error, the per-call scratch copy below serves
                }
            }
            if (bs.d_endo && bs.endo_first == first && bs.endo_n == n_real && bs.endo_k == endo_k) {
                d_phi = reinterpret_cast<const Affine<F>*>(bs.d_endo);
                phi_owner = false;
                phi_cached = true;
            }
        }
        if (glv && phi_owner) {
            if ((rc = zl_scratch_get(ctx, phi_slot, (size_t)(endo_k - 1) * n_real * sizeof(Affine<F>), &p))) return rc;
            d_phi = reinterpret_cast<const Affine<F>*>(p);
        }
        return ZL_OK;
    }
    int sort(zl_ctx* ctx, hipStream_t st) {
        // the bucket counters are written in full by the LDS path (k_msm_slice_prefix) and by the wide path (k_msm_fine_hist); only the
        // global-atomics sort counts into them
        if (!wide && c > 16) ZL_HIP(ctx, hipMemsetAsync(d_counts, 0, (size_t)(NB + 1) * 4, st));
        hipLaunchKernelGGL(k_msm_zero_words, dim3(1), dim3(64), 0, st, d_big_count, 8u);  // big, ones, giant counts, bad-scalar flag; [4..5]: oversized sub-group queue head (u64); [6]: k_msm_ones' ticket
        const uint32_t nblk = (uint32_t)((n + 255) / 256);
        // GLV front end: half-scalars behind the sort temporaries, phi image of the bases (once per call for a batch over one key)
        const uint32_t* sc_eff = sc;
        const uint8_t* inf_eff = d_inf;
        uint32_t* bad_eff = d_bad_scalar;
        if (cover) {  // the recoder reads the caller's scalars and splits them itself; only the phi image is left of the front end
            if constexpr (G::GLV && G::ENDO_K == 2) {
                if (phi_owner)
                    hipLaunchKernelGGL((k_glv_phi<G>), dim3((uint32_t)((n_real + 127) / 128)), dim3(128), 0, st, d_bases, (uint32_t)n_real, const_cast<Affine<F>*>(d_phi));
            }
        } else if (glv) {
            d_vs = reinterpret_cast<uint32_t*>(d_sort_a + lay.vs);
            if constexpr (G::GLV && G::ENDO_K == 2) {
                if constexpr (G::GLVP::LATTICE)
                    hipLaunchKernelGGL((k_glv_split_lattice<typename G::GLVP>), dim3((uint32_t)((n_real + 255) / 256)), dim3(256), 0, st, sc, (uint32_t)n_real, d_inf, d_vs, (int)G::SC_BITS, d_bad_scalar);
                else
                    hipLaunchKernelGGL((k_glv_split<typename G::GLVP>), dim3((uint32_t)((n_real + 255) / 256)), dim3(256), 0, st, sc, (uint32_t)n_real, d_inf, d_vs, (int)G::SC_BITS, d_bad_scalar);
                if (phi_owner)
                    hipLaunchKernelGGL((k_glv_phi<G>), dim3((uint32_t)((n_real + 127) / 128)), dim3(128), 0, st, d_bases, (uint32_t)n_real, const_cast<Affine<F>*>(d_phi));
            } else if constexpr (G::GLV && G::ENDO_K == 4) {
                if constexpr (G::GLVP::LATTICE)
                    hipLaunchKernelGGL((k_gls_split_lattice<typename G::GLVP>), dim3((uint32_t)((n_real + 255) / 256)), dim3(256), 0, st, sc, (uint32_t)n_real, d_inf, d_vs, (int)G::SC_BITS, d_bad_scalar);
                else
                    hipLaunchKernelGGL((k_gls_split<typename G::GLVP>), dim3((uint32_t)((n_real + 255) / 256)), dim3(256), 0, st, sc, (uint32_t)n_real, d_inf, d_vs, (int)G::SC_BITS, d_bad_scalar);
                if (phi_owner)
                    hipLaunchKernelGGL((k_gls_psi<G>), dim3((uint32_t)((n_real + 63) / 64)), dim3(64), 0, st, d_bases, (uint32_t)n_real, const_cast<Affine<F>*>(d_phi));
            }
            sc_eff = d_vs;
            inf_eff = nullptr;  // the split already dropped the scalars of bases at infinity
            bad_eff = nullptr;  // ... and checked the scalars' width
        }
        const int glv_i = glv ? 1 : 0;
        // per call, not once per process: the attribute is per device and a process may own several contexts
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_msm_hist_lds), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_msm_scatter_range), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        if (wide) sort_wide(st, sc_eff, inf_eff, bad_eff, glv_i);
        else if (sort_is_lds()) sort_lds(st, sc_eff, inf_eff, bad_eff, nblk, glv_i);
        else sort_atomics(st, nblk);
        ZL_HIP(ctx, hipGetLastError());
        return ZL_OK;
    }
    // ---- three-level counting sort over (window, bucket) ids: the merged set of a table, or W sets of plain wide windows (c = 17 .. 20; GLS quarter-scalars at c = 16)
    void sort_wide(hipStream_t st, const uint32_t* sc_eff, const uint8_t* inf_eff, uint32_t* bad_eff, int glv_i) {
        const zl_bases& bs = *bsp;
        const uint32_t nslices = lay.nslices, per_slice = lay.per_slice, P = lay.P, pscan_blocks = lay.pscan_blocks;
        uint16_t* d_lo16 = (uint16_t*)d_sort_a;
        uint8_t* d_hi8 = (uint8_t*)(d_sort_a + lay.hi8);
        uint16_t* d_part_lo = (uint16_t*)(d_sort_a + lay.part_lo);
        uint32_t* d_part_idx = (uint32_t*)(d_sort_a + lay.part_idx);
        uint32_t* d_pcounts = (uint32_t*)(d_sort_a + lay.pcounts);
        uint32_t* d_poff = d_pcounts + P;            // P + 1 entries (total at [P])
        uint32_t* d_pblock = d_poff + P + 1;
        // the recoder counts the first partition's histogram as it goes (into zeroed counters): blocks of up to 8192 scalars inside one slice, so that a block sends
        // one atomic per (window, group) it met -- 2048 blocks at 2^24 -- and still one block per 256 scalars below 2^19, where the launch is latency
        const uint32_t span = 256u * std::min<uint32_t>(32u, std::max<uint32_t>(1u, (uint32_t)(n >> 19)));
        (void)hipMemsetAsync(d_pcounts, 0, (size_t)P * 4, st);
        if (cover) {
            // blocks over the n_real scalars; a block's records of either half meet at most two slices of the 2 n_real records (zl_msm_sort.h)
            const uint32_t cspan = nslices > 1 ? std::min<uint32_t>(span, per_slice / 256u * 256u) : span;
            hipLaunchKernelGGL(k_msm_recode_cover, dim3((uint32_t)((n_real + cspan - 1) / cspan)), dim3(256), zl_recode_cover_lds(Gn), st, sc_eff, (uint32_t)n_real, cv, d_lo16, d_hi8,
                               d_ones_list, d_ones_count, inf_eff, (int)G::SC_BITS, bad_eff, Gn, per_slice, cspan, nslices, d_pcounts);
        } else
        hipLaunchKernelGGL(k_msm_recode_wide,dim3((per_slice + span - 1) / span, nslices), dim3(256), zl_recode_wide_lds(Gn, (uint32_t)W, pre ? 0u : (H >> 15)), st, sc_eff, (uint32_t)n, c, W, pre ? 0u : (H >> 15), spread_t, glv_i,
                           d_lo16, d_hi8, d_ones_list, d_ones_count, inf_eff, sc_bits, bad_eff, Gn, per_slice, span, nslices, d_pcounts);
        hipLaunchKernelGGL(k_scan_block_sums, dim3(pscan_blocks), dim3(SCAN_BLOCK), 0, st, d_pcounts, P, d_pblock);
        hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, st, d_pblock, pscan_blocks, d_poff + P, (const uint32_t*)nullptr);
        hipLaunchKernelGGL(k_scan_apply, dim3(pscan_blocks), dim3(SCAN_BLOCK), 0, st, d_pcounts, P, d_pblock, d_poff, d_pcounts);
        hipLaunchKernelGGL(k_msm_part_scatter_st, dim3(nslices, W), dim3(256), 0, st, d_lo16, d_hi8, (uint32_t)n, (uint32_t)W, Gn, per_slice, nslices, d_poff,
                           pre ? (uint32_t)bs.n : 0u, pre ? (uint32_t)first : 0u, d_part_lo, d_part_idx);  // plain: d_bases already starts at `first`
        const uint32_t gstride = (uint32_t)W * nslices;  // counters per group
        // level 2: 128 sub-groups (256 buckets each) per group; level 3: LDS-staged sort per sub-group
        const uint32_t SG = Gn * 128;
        const uint32_t fsl = lay.fsl, P2 = lay.P2, p2scan_blocks = lay.p2scan_blocks;
        uint16_t* d_lo2 = (uint16_t*)d_sort_b;
        uint32_t* d_idx2 = (uint32_t*)(d_sort_b + lay.idx2);
        uint32_t* d_c2 = (uint32_t*)(d_sort_b + lay.counts2);
        uint32_t* d_off2 = d_c2 + P2;  // P2 + 1
        uint32_t* d_blk2 = d_off2 + P2 + 1;
        hipLaunchKernelGGL(k_msm_sub_hist, dim3(fsl, Gn), dim3(256), 0, st, d_part_lo, d_poff, Gn, gstride, d_poff + P, fsl, d_c2);
        hipLaunchKernelGGL(k_scan_block_sums, dim3(p2scan_blocks), dim3(SCAN_BLOCK), 0, st, d_c2, P2, d_blk2);
        hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, st, d_blk2, p2scan_blocks, d_off2 + P2, (const uint32_t*)nullptr);
        hipLaunchKernelGGL(k_scan_apply, dim3(p2scan_blocks), dim3(SCAN_BLOCK), 0, st, d_c2, P2, d_blk2, d_off2, d_c2);
        hipLaunchKernelGGL(k_msm_sub_scatter_st, dim3(fsl, Gn), dim3(256), 0, st, d_part_lo, d_part_idx, d_poff, Gn, gstride, d_poff + P, fsl, d_off2, d_lo2,
                           d_idx2);
        hipLaunchKernelGGL(k_msm_fine_hist, dim3(SG), dim3(256), 0, st, d_lo2, d_off2, SG, fsl, d_off2 + P2, d_counts);
        hipLaunchKernelGGL(k_scan_block_sums, dim3(scan_blocks), dim3(SCAN_BLOCK), 0, st, d_counts, NB, d_block_sums);
        hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, st, d_block_sums, scan_blocks, d_offsets + NB, (const uint32_t*)d_bad_scalar);
        hipLaunchKernelGGL(k_scan_apply, dim3(scan_blocks), dim3(SCAN_BLOCK), 0, st, d_counts, NB, d_block_sums, d_offsets, d_cursor);
        const uint32_t cap = fine_cap();
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_msm_fine_sort), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        hipLaunchKernelGGL(k_msm_fine_sort, dim3(SG), dim3(fine_threads()), (size_t)(256 + cap) * 4, st, d_lo2, d_idx2, d_off2, SG, fsl, d_off2 + P2, d_offsets, cap,
                           d_entries, d_bigsg_head, d_bigsg_items);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_msm_fine_sort_big), hipFuncAttributeMaxDynamicSharedMemorySize, ZL_BT * 4);
        hipLaunchKernelGGL(k_msm_fine_sort_big, dim3(512), dim3(1024), (size_t)ZL_BT * 4, st, d_lo2, d_idx2, d_off2, SG, fsl, d_off2 + P2, d_bigsg_head,
                           d_bigsg_items, d_cursor, d_entries);
    }
    // ---- LDS counting sort (c <= 16): recode once (u16 digits), per-(slice, window) LDS histograms, slice prefix, scan, range-owned scatter
    void sort_lds(hipStream_t st, const uint32_t* sc_eff, const uint8_t* inf_eff, uint32_t* bad_eff, uint32_t nblk, int glv_i) {
        const uint32_t nslices = lay.nslices, per_slice = lay.per_slice;
        uint16_t* d_digits = (uint16_t*)d_sort_a;
        uint32_t* d_slice_counts = (uint32_t*)(d_sort_a + lay.slice_counts);
        hipLaunchKernelGGL(k_msm_recode, dim3(nblk), dim3(256), 0, st, sc_eff, (uint32_t)n, c, W, spread_t, glv_i, d_digits, d_ones_list, d_ones_count, inf_eff, sc_bits, bad_eff);
        hipLaunchKernelGGL(k_msm_hist_lds, dim3(nslices, W), dim3(1024), (size_t)H * 4, st, d_digits, (uint32_t)n, H, per_slice, NB, d_slice_counts);
        if (lds_prefix_small()) {
            hipLaunchKernelGGL(k_msm_prefix_small, dim3(1), dim3(1024), ((size_t)NB + NB / 16 + 16) * 4, st, d_slice_counts, NB, nslices, d_offsets, d_cursor, (const uint32_t*)d_bad_scalar);
        } else {
        hipLaunchKernelGGL(k_msm_slice_prefix, dim3((NB + 255) / 256), dim3(256), 0, st, d_slice_counts, NB, nslices, d_counts);
        hipLaunchKernelGGL(k_scan_block_sums, dim3(scan_blocks), dim3(SCAN_BLOCK), 0, st, d_counts, NB, d_block_sums);
        hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, st, d_block_sums, scan_blocks, d_offsets + NB, (const uint32_t*)d_bad_scalar);
        hipLaunchKernelGGL(k_scan_apply, dim3(scan_blocks), dim3(SCAN_BLOCK), 0, st, d_counts, NB, d_block_sums, d_offsets, d_cursor);
        }
        const uint32_t ranges = lds_ranges();
        const uint32_t RB = (H + ranges - 1) / ranges;
        // (the digit row of a window can be walked by `parts` blocks, slice-aligned: measured 1 = 2 = 4 = 8 at 2^18 .. 2^21 -- the kernel is bound by
        // its 4-byte scattered stores, 16.8 M of them in 0.19 ms at 2^20, not by the length of the row, the load latency or the LDS atomics)
        const uint32_t parts = 1;
        hipLaunchKernelGGL(k_msm_scatter_range, dim3(8 * ((W + 7) / 8), ranges, parts), dim3(1024), (size_t)RB * 4, st, d_digits, (uint32_t)n, H, RB, d_offsets, d_entries,
                           (const uint32_t*)d_slice_counts, NB, nslices, per_slice, parts, (uint32_t)W);
    }
    // ---- wide windows without a table beyond 255 sort groups (forced plain c >= 21): histogram / scatter with global atomics
    void sort_atomics(hipStream_t st, uint32_t nblk) {
        // wide windows without a table: histogram / scatter with global atomics
        hipLaunchKernelGGL((k_msm_digits<0>), dim3(nblk), dim3(256), 0, st, sc, (uint32_t)n, c, W, d_counts, (uint32_t*)nullptr, d_ones_list, d_ones_count, d_inf, (int)G::SC_BITS, d_bad_scalar);
        hipLaunchKernelGGL(k_scan_block_sums, dim3(scan_blocks), dim3(SCAN_BLOCK), 0, st, d_counts, NB, d_block_sums);
        hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, st, d_block_sums, scan_blocks, d_offsets + NB, (const uint32_t*)d_bad_scalar);
        hipLaunchKernelGGL(k_scan_apply, dim3(scan_blocks), dim3(SCAN_BLOCK), 0, st, d_counts, NB, d_block_sums, d_offsets, d_cursor);
        hipLaunchKernelGGL((k_msm_digits<1>), dim3(nblk), dim3(256), 0, st, sc, (uint32_t)n, c, W, d_cursor, d_entries, d_ones_list, d_ones_count, d_inf, (int)G::SC_BITS, d_bad_scalar);
    }
    static constexpr bool pair_ok() { return G::COORDS == 2 && !std::is_void<typename PairBase<F>::type>::value; }  // an Fq2 group on 28-bit limbs: the lane-pair kernels exist
    int accumulate(zl_ctx* ctx, hipStream_t st) {
        static_assert(G::COORDS == 1 || pair_ok(), "every Fq2 group runs on 28-bit limbs: its MSM kernels are the lane-pair ones");
        const bool quad = acc_quad();
        if constexpr (pair_ok()) {  // Fq2 groups (zl_fq2pair.h): eight lanes per chunk, else two lanes per chunk at two waves per SIMD
            if (quad)
                hipLaunchKernelGGL((k_msm_accumulate_pair<G, true>), dim3((nchunks + 7) / 8), dim3(64), 0, st, d_entries, d_offsets, NB, d_bases, d_buckets, d_partials, ZL_CHUNK,
                                   glv ? d_phi : d_bases, glv ? (uint32_t)n_real : 0xFFFFFFFFu);
            else
                hipLaunchKernelGGL((k_msm_accumulate_pair<G, false>), dim3((nchunks + 31) / 32), dim3(64), 0, st, d_entries, d_offsets, NB, d_bases, d_buckets, d_partials, ZL_CHUNK,
                                   glv ? d_phi : d_bases, glv ? (uint32_t)n_real : 0xFFFFFFFFu);
        } else {
            if (quad)
                hipLaunchKernelGGL((k_msm_accumulate_quad<G>), dim3((4 * nchunks + ZL_ACC_BLOCK - 1) / ZL_ACC_BLOCK), dim3(ZL_ACC_BLOCK), 0, st, d_entries, d_offsets, NB, d_bases, d_buckets, d_partials, ZL_CHUNK,
                                   glv ? d_phi : d_bases, glv ? (uint32_t)n_real : 0xFFFFFFFFu, d_chunk_head);
#ifdef ZL_MEASURE
            else if (ctx->acc_clk && (size_t)((nchunks + ZL_ACC_BLOCK - 1) / ZL_ACC_BLOCK) * 32 <= ctx->acc_clk_cap) {  // armed by the measurement hook zl_test_acc_clock only
                ctx->acc_clk_waves = (nchunks + ZL_ACC_BLOCK - 1) / ZL_ACC_BLOCK;
                hipLaunchKernelGGL((k_msm_accumulate_clk<G>), dim3((nchunks + ZL_ACC_BLOCK - 1) / ZL_ACC_BLOCK), dim3(ZL_ACC_BLOCK), 0, st, d_entries, d_offsets, NB, d_bases, d_buckets, d_partials, ZL_CHUNK,
                                   glv ? d_phi : d_bases, glv ? (uint32_t)n_real : 0xFFFFFFFFu, d_chunk_head, (unsigned long long*)ctx->acc_clk,
                                   zl_tune("ZL_TUNE_ACC_CLK_IDX_BITS", 31) >= 31 ? 0x7fffffffu : ((1u << zl_tune("ZL_TUNE_ACC_CLK_IDX_BITS", 31)) - 1u));
            }
#endif
            else
                hipLaunchKernelGGL((k_msm_accumulate<G>), dim3((nchunks + ZL_ACC_BLOCK - 1) / ZL_ACC_BLOCK), dim3(ZL_ACC_BLOCK), 0, st, d_entries, d_offsets, NB, d_bases, d_buckets, d_partials, ZL_CHUNK,
                                   glv ? d_phi : d_bases, glv ? (uint32_t)n_real : 0xFFFFFFFFu, d_chunk_head);
        }
        ZL_HIP(ctx, hipGetLastError());
        return ZL_OK;
    }
    int tail(zl_ctx* ctx, hipStream_t st) {
        // four lanes per group operation in every tail launch that does not fill the machine, one lane (Fq2: a lane pair) in those that do
        const uint32_t quad_max = tail_quad_max();
        const bool by_cuts = this->by_cuts();
        if (by_cuts) hipLaunchKernelGGL((k_msm_fill_empty<G>), dim3((NB + 255) / 256), dim3(256), 0, st, d_offsets, NB, d_buckets);
        if constexpr (pair_ok()) {
            if (by_cuts)
                hipLaunchKernelGGL((k_msm_merge_cuts_pair<G>), dim3((nchunks + 31) / 32), dim3(64), 0, st, d_offsets, NB, d_buckets, d_partials, d_big_list, d_big_count, d_giant_list, d_giant_count, ZL_CHUNK, big_span, nchunks);
            else if (NB > quad_max)
                hipLaunchKernelGGL((k_msm_merge_pair<G, false>), dim3((NB + 31) / 32), dim3(64), 0, st, d_offsets, NB, d_buckets, d_partials, d_big_list, d_big_count, d_giant_list, d_giant_count, ZL_CHUNK, big_span);
            else
                hipLaunchKernelGGL((k_msm_merge_pair<G, true>), dim3((NB + 7) / 8), dim3(64), 0, st, d_offsets, NB, d_buckets, d_partials, d_big_list, d_big_count, d_giant_list, d_giant_count, ZL_CHUNK, big_span);
        } else {
            if (by_cuts)
                hipLaunchKernelGGL((k_msm_merge_cuts<G>), dim3((nchunks + 63) / 64), dim3(64), 0, st, d_offsets, d_chunk_head, NB, d_buckets, d_partials, d_big_list, d_big_count, d_giant_list, d_giant_count, ZL_CHUNK, big_span, nchunks);
            else if (NB > quad_max)  // (a single chunk)
                hipLaunchKernelGGL((k_msm_merge<G>), dim3((NB + 63) / 64), dim3(64), 0, st, d_offsets, NB, d_buckets, d_partials, d_big_list, d_big_count, d_giant_list, d_giant_count, ZL_CHUNK, big_span);
            else
                hipLaunchKernelGGL((k_msm_merge<G, true>), dim3((4 * NB + 63) / 64), dim3(64), 0, st, d_offsets, NB, d_buckets, d_partials, d_big_list, d_big_count, d_giant_list, d_giant_count, ZL_CHUNK, big_span);
        }
        const bool may_big = this->may_big(), may_giant = this->may_giant();
        if constexpr (pair_ok()) {  // Fq2 groups: the block-tree kernels of the heavy buckets on lane pairs
            if (may_big) hipLaunchKernelGGL((k_msm_merge_big_pair<G>), dim3(std::min<uint32_t>(max_big, 1024)), dim3(2 * TreeLanes<G>::N), TreeLanes<G>::N * sizeof(X), st, d_offsets, d_buckets,
                               d_partials, d_big_list, d_big_count, ZL_CHUNK);
            if (may_giant) hipLaunchKernelGGL((k_msm_merge_giant_pair<G>), dim3(std::min<uint32_t>(max_giant, 16) * ZL_GIANT_PARTS), dim3(2 * TreeLanes<G>::N), TreeLanes<G>::N * sizeof(X), st,
                               d_offsets, d_giant_tmp, d_partials, d_giant_list, d_giant_count, ZL_CHUNK);
            if (may_giant) hipLaunchKernelGGL((k_msm_merge_giant2_pair<G>), dim3(std::min<uint32_t>(max_giant, 64)), dim3(2 * ZL_GIANT_PARTS), 0, st, d_buckets, d_giant_tmp, d_giant_list, d_giant_count);
        } else {
            if (may_big) hipLaunchKernelGGL((k_msm_merge_big<G>), dim3(std::min<uint32_t>(max_big, 1024)), dim3(TreeLanes<G>::N), TreeLanes<G>::N * sizeof(X), st, d_offsets, d_buckets,
                           d_partials, d_big_list, d_big_count, ZL_CHUNK);
            if (may_giant) hipLaunchKernelGGL((k_msm_merge_giant<G>), dim3(std::min<uint32_t>(max_giant, 16) * ZL_GIANT_PARTS), dim3(TreeLanes<G>::N), TreeLanes<G>::N * sizeof(X), st,
                           d_offsets, d_giant_tmp, d_partials, d_giant_list, d_giant_count, ZL_CHUNK);
            if (may_giant) hipLaunchKernelGGL((k_msm_merge_giant2<G>), dim3((max_giant + 63) / 64), dim3(64), 0, st, d_buckets, d_giant_tmp, d_giant_list, d_giant_count);
        }
        // scalar-1 bases: window-0 table entries are the bases themselves
        hipLaunchKernelGGL((k_msm_ones<G>), dim3(ZL_ONES_BLOCKS), dim3(TreeLanes<G>::N), TreeLanes<G>::N * sizeof(X), st, d_ones_list, d_ones_count,
                           pre ? d_bases + first : d_bases, d_ones_parts, glv ? d_phi : d_bases, glv ? (uint32_t)n_real : 0xFFFFFFFFu,
                           d_sets + (size_t)SETS * roots_per_set, d_big_count + 6, (const uint32_t*)(d_offsets + NB));  // (+ the final sum and the two status words: see the kernel)
        {
            const uint32_t fset = spread_t >= 0 ? (uint32_t)(W - 1) : 0xFFFFFFFFu, flog = (uint32_t)std::max(spread_t, 0);
            const uint32_t leaves = SETS * red_blocks;
            X* cur = red_levels == 0 ? d_sets : d_segs;
            if constexpr (pair_ok()) {
                if (leaves > quad_max)
                    hipLaunchKernelGGL((k_msm_reduce_level0_pair<G, false>), dim3((leaves + 31) / 32), dim3(64), 0, st, d_buckets, H, red_g0, red_blocks, leaves, fset, flog, cur);
                else
                    hipLaunchKernelGGL((k_msm_reduce_level0_pair<G, true>), dim3((leaves + 7) / 8), dim3(64), 0, st, d_buckets, H, red_g0, red_blocks, leaves, fset, flog, cur);
            } else {
                if (leaves > quad_max)
                    hipLaunchKernelGGL((k_msm_reduce_level0<G>), dim3((leaves + 63) / 64), dim3(64), 0, st, d_buckets, H, red_g0, red_blocks, leaves, fset, flog, cur);
                else
                    hipLaunchKernelGGL((k_msm_reduce_level0<G, true>), dim3((4 * leaves + 63) / 64), dim3(64), 0, st, d_buckets, H, red_g0, red_blocks, leaves, fset, flog, cur);
            }
            for (uint32_t lv = 1; lv <= red_levels; lv++) {
                const uint32_t nodes = red_blocks >> lv, lanes = SETS * nodes * (lv + 2);
                X* nxt = lv == red_levels ? d_sets : ((lv & 1) ? d_stage1 : d_segs);
                if constexpr (pair_ok()) {
                    if (lanes > quad_max)
                        hipLaunchKernelGGL((k_msm_reduce_tree_pair<G, false>), dim3((lanes + 31) / 32), dim3(64), 0, st, cur, nxt, lv, nodes, lanes);
                    else
                        hipLaunchKernelGGL((k_msm_reduce_tree_pair<G, true>), dim3((lanes + 7) / 8), dim3(64), 0, st, cur, nxt, lv, nodes, lanes);
                } else {
                    if (lanes > quad_max) {  // adding blocks, then the blocks that copy the top channels
                        uint32_t add_blocks, copy_blocks;
                        zl_tree_blocks<G>(lv, SETS * nodes, add_blocks, copy_blocks);
                        hipLaunchKernelGGL((k_msm_reduce_tree<G>), dim3(add_blocks + copy_blocks), dim3(64), 0, st, cur, nxt, lv, nodes, lanes);
                    }
                    else
                        hipLaunchKernelGGL((k_msm_reduce_tree<G, true>), dim3((4 * lanes + 63) / 64), dim3(64), 0, st, cur, nxt, lv, nodes, lanes);
                }
                cur = nxt;
            }
        }
        ZL_HIP(ctx, hipGetLastError());
        ZL_HIP(ctx, hipMemcpyAsync(hw, d_sets, sizeof(X) * ((size_t)SETS * roots_per_set + 1) + 8, hipMemcpyDeviceToHost, st));  // root channels, scalar-1 sum, the two status words
        return ZL_OK;
    }
    // The window sum of set w is V_w = A_w + g0 * sum_b 2^b S_(w,b) (the root channels T, A, S_0 .. of its reduction tree); the result is
    // sum_w 2^(c w) V_w (the table of a precomputed handle already carries that factor: one set, w = 0) + the scalar-1 bases.
    //   stage 1  every V_w by its own short Horner over the bit positions of the window (<= c - 2 doublings, levels + 1 additions): the
    //            sets are independent -> zl_pool, one task per set
    //   stage 2  one serial Horner over the sets, high to low: c doublings + one addition per set (the ~c W doublings every window
    //            method needs)
    // (Rounds 1-2 ran ONE Horner over all bit positions on one thread: the same ~c W doublings, but all (levels + 2) W additions
    // serial as well: 0.40 ms for BLS12-381 G1 at c = 16 against ~0.2 ms now.)
    X window_value(int w) const {
        const X* root = hw + (size_t)w * roots_per_set;  // channels: T, A, S_0 ..
        X v = X::inf();
        const int top = (int)red_lg0 + (int)red_levels - 1;  // highest position inside the window that carries a channel
        for (int off = std::max(top, 0); off >= 0; off--) {
            if (off != std::max(top, 0)) zl::dbl_inplace(v);
            const int bsel = off - (int)red_lg0;
            if (bsel >= 0 && bsel < (int)red_levels) {
                const bool skipped = spread_t >= 0 && w == (int)SETS - 1 && off >= spread_t && !pre;  // spread top window: bits from spread_t on carry no weight
                if (!skipped) zl::add_full(v, root[2 + bsel]);
            }
            if (off == 0) zl::add_full(v, root[1]);
        }
        return v;
    }
    X finish(bool parallel = true, double* values_us = nullptr) const {  // values_us (developer trace): time of stage 1
        std::vector<X> V(SETS);
        const auto t0 = std::chrono::steady_clock::now();
        if (parallel && SETS >= 4) zl_pool_get().parallel_for(SETS, [&](size_t w) { V[w] = window_value((int)w); });
        else for (uint32_t w = 0; w < SETS; w++) V[w] = window_value((int)w);
        if (values_us) *values_us = (double)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count() / 1e3;
        if (cover) {
            // Exact-cover plan: set j of window w holds the digits m in (j 2^set_log, (j + 1) 2^set_log] under the weights m - j 2^set_log, so the window sum is
            // sum_j V_j + 2^set_log sum_j j T_j with T_j the set's total (root channel 0); sum_j j T_j = sum_(i >= 1) sum_(j >= i) T_j costs two additions per set.
            // The windows then fold high to low, width[w] doublings between window w + 1 and window w.
            X total = X::inf();
            for (int w = (int)cv.windows - 1; w >= 0; w--) {
                if (w != (int)cv.windows - 1) zl::dbl_n(total, (int)cv.width[w]);
                X run = X::inf(), extra = X::inf(), plain = X::inf();
                for (int j = (int)cv.sets[w] - 1; j >= 0; j--) {
                    const uint32_t s = cv.base[w] + (uint32_t)j;
                    zl::add_full(plain, V[s]);
                    if (j >= 1) {
                        zl::add_full(run, hw[(size_t)s * roots_per_set]);
                        zl::add_full(extra, run);
                    }
                }
                zl::dbl_n(extra, (int)cv.set_log);
                zl::add_full(total, plain);
                zl::add_full(total, extra);
            }
            zl::add_full(total, hw[(size_t)SETS * roots_per_set]);
            return total;
        }
        X total = V[SETS - 1];
        for (int w = (int)SETS - 2; w >= 0; w--) {
            zl::dbl_n(total, c);  // c doublings in Jacobian coordinates
            zl::add_full(total, V[w]);
        }
        zl::add_full(total, hw[(size_t)SETS * roots_per_set]);
        return total;
    }
};
