// zl_ctx.h -- internal context shared by the MSM / NTT translation units (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include <atomic>
#include <functional>
#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <vector>
#include "../../include/zl_backend_ext.h"
#include "zl_curve.h"
#include "zl_pool.h"

#define ZL_HIP(ctx, call)                                   \
    do {                                                    \
        hipError_t e_ = (call);                             \
        if (e_ != hipSuccess) {                             \
            (ctx)->last_hip = (int)e_;                      \
            return e_ == hipErrorOutOfMemory ? ZL_ENOMEM : ZL_EHIP; \
        }                                                   \
    } while (0)

// ---- group configurations ---------------------------------------------------------------------------------
struct BlsG1 {
    static constexpr int ID = 0;
    using FqP = BLS12_381_Fq;
    using FrP = BLS12_381_Fr;
    using F = Fp28<BLS12_381_Fq28, BLS12_381_Fq>;  // 14 x 28-bit lazily reduced limbs (zl_field28.h): +30 % multiplier throughput
    using C = BLS12_381_G1;
    static constexpr int SC_BITS = 255;
    static constexpr int FQ64 = 6;     // u64 limbs per Fq element in the ABI layouts
    static constexpr int COORDS = 1;   // Fq elements per coordinate
    static constexpr bool GLV = true;  // plain MSMs split every scalar with the endomorphism (x, y) -> (beta x, y) = [lambda](x, y)
    static constexpr int ENDO_K = 2;   // ... into two 127-bit halves
    using GLVP = BLS12_381_GLV;
    ZL_HD static F glv_beta() { uint32_t w[FqP::N]; for (int i = 0; i < FqP::N; i++) w[i] = GLVP::beta(i); return FieldIO<F>::load_mont32(w); }
    ZL_HD static F gen_x() { uint32_t w[FqP::N]; for (int i = 0; i < FqP::N; i++) w[i] = C::gx(i); return FieldIO<F>::load_mont32(w); }
    ZL_HD static F gen_y() { uint32_t w[FqP::N]; for (int i = 0; i < FqP::N; i++) w[i] = C::gy(i); return FieldIO<F>::load_mont32(w); }
    ZL_HD static F coeff_b() { uint32_t w[FqP::N]; for (int i = 0; i < FqP::N; i++) w[i] = C::b(i); return FieldIO<F>::load_mont32(w); }
};
struct BnG1 {
    static constexpr int ID = 1;
    using FqP = BN254_Fq;
    using FrP = BN254_Fr;
    using F = Fp28<BN254_Fq28, BN254_Fq>;  // round 4: 10 x 28-bit lazily reduced limbs like BLS12-381 (zl_field28.h)
    using C = BN254_G1;
    static constexpr int SC_BITS = 254;
    static constexpr int FQ64 = 4;
    static constexpr int COORDS = 1;
    static constexpr bool GLV = true;  // round 6: the same endomorphism split as BLS12-381 G1, with the two-dimensional lattice decomposition (BN254_GLV, k_glv_split_lattice)
    static constexpr int ENDO_K = 2;
    using GLVP = BN254_GLV;
    ZL_HD static F glv_beta() { uint32_t w[FqP::N]; for (int i = 0; i < FqP::N; i++) w[i] = GLVP::beta(i); return FieldIO<F>::load_mont32(w); }
    ZL_HD static F gen_x() { uint32_t w[FqP::N]; for (int i = 0; i < FqP::N; i++) w[i] = C::gx(i); return FieldIO<F>::load_mont32(w); }
    ZL_HD static F gen_y() { uint32_t w[FqP::N]; for (int i = 0; i < FqP::N; i++) w[i] = C::gy(i); return FieldIO<F>::load_mont32(w); }
    ZL_HD static F coeff_b() { uint32_t w[FqP::N]; for (int i = 0; i < FqP::N; i++) w[i] = C::b(i); return FieldIO<F>::load_mont32(w); }
};
template <class C2, class FqP_, class FrP_, class F_, class GLS_, int SCB, int FQ64_, int ID_>
struct G2Cfg {
    static constexpr int ID = ID_;
    using FqP = FqP_;
    using FrP = FrP_;
    using F = F_;
    static constexpr int SC_BITS = SCB;
    static constexpr int FQ64 = FQ64_;
    static constexpr int COORDS = 2;
    // GLS: the untwist-Frobenius-twist endomorphism psi acts on G2 as [lambda] with lambda^4 - lambda^2 + 1 = 0 (mod r); a scalar becomes four signed
    // quarter-scalars of GLVP::QUARTER_BITS bits over P, psi(P), psi^2(P), psi^3(P).  BLS12-381 (ID 2): lambda = z = -|z| and r < |z|^4, the quarters are the
    // base-|z| digits with alternating signs (k_gls_split).  BN254 (ID 3): lambda = 6 x^2, a four-dimensional lattice split with a sign per quarter
    // (BN254_GLS, k_gls_split_lattice).  GLVP carries the split parameters and the psi constants of the curve.
    static constexpr bool GLV = true;
    static constexpr int ENDO_K = 4;
    using GLVP = GLS_;
    ZL_HD static F psi_x() { return mk(GLVP::psi_x0, GLVP::psi_x1); }
    ZL_HD static F psi_y() { return mk(GLVP::psi_y0, GLVP::psi_y1); }
    ZL_HD static F mk(uint32_t (*f0)(int), uint32_t (*f1)(int)) {  // two components as arkworks' Montgomery words
        uint32_t w[2 * FqP::N];
        for (int i = 0; i < FqP::N; i++) { w[i] = f0(i); w[FqP::N + i] = f1(i); }
        return FieldIO<F>::load_mont32(w);
    }
    ZL_HD static F gen_x() { return mk(C2::gx0, C2::gx1); }
    ZL_HD static F gen_y() { return mk(C2::gy0, C2::gy1); }
    ZL_HD static F coeff_b() { return mk(C2::b0, C2::b1); }
};
// G2 on the lazily reduced 28-bit fields (Fq2 products as dual scans, zl_field28.h): 14 limbs per component for BLS12-381, 10 for BN254
using BlsG2 = G2Cfg<BLS12_381_G2, BLS12_381_Fq, BLS12_381_Fr, Fp2L<Fp28<BLS12_381_Fq28, BLS12_381_Fq>>, BLS12_381_GLS, 255, 6, 2>;
using BnG2 = G2Cfg<BN254_G2, BN254_Fq, BN254_Fr, Fp2L<Fp28<BN254_Fq28, BN254_Fq>>, BN254_GLS, 254, 4, 3>;  // round 4: like BLS12-381 G2, on 10 limbs

// ---- context ----------------------------------------------------------------------------------------------
struct zl_bases {
    void* d_pts = nullptr;  // Affine<F>[n], Montgomery
    void* d_table = nullptr;  // optional Affine<F>[W][n]: 2^(c w) P_i (zl_bases_precompute)
    int precomp_c = 0;
    void* d_inf = nullptr;   // optional uint8[n]: 1 = the point at infinity (present only when the handle holds at least one)
    size_t n_inf = 0;
    size_t n = 0;
    int curve = 0, group = 0;
    // endomorphism images of points [endo_first, endo_first + endo_n) (GLV: phi(P); GLS: psi, psi^2, psi^3), built by the first small MSM over
    // that range and kept with the handle: a proving key's queries are always used with the same range
    mutable void* d_endo = nullptr;
    mutable size_t endo_first = 0, endo_n = 0;
    mutable int endo_k = 0;
    mutable std::vector<uint64_t> first_xy;  // canonical affine words of point 0, fetched once (Groth16: the z_0 = 1 term of a / b queries)
    // Groth16 per-key state hung on the l_query handle of a proving key (zl_groth16.hip: host tables of the key's fixed points, the folded C query of small
    // proofs); built on the first proof over the key under zl_bases_cache_mutex, released with the handle
    mutable std::shared_ptr<void> g16_cache;
};
struct zl_scratch {
    void* p = nullptr;
    size_t cap = 0;
};
// ---- the map of zl_ctx::scratch: every grow-only device block of a ctx, by owner --------------------------------------------------------
// A ctx is SINGLE-CALLER and every entry point drains the ctx's streams before it returns, so a block is only ever shared between calls:
//   * MSM buffer sets 0..3 (ZL_MSM_SET below).  A single call uses set 0; the three-phase pipeline rotates sets 0..2 and sorts every job in
//     ZL_SLOT_SORT_A / _B (the sorts run in order on one stream); small jobs side by side take sets 0..3, each with its own sort pair.
//   * ZL_SLOT_PHI_ONE_KEY: the endomorphism image of the bases when the jobs of a call share one key (single call, pipelined batch over one
//     handle); a heterogeneous or side-by-side batch keeps one image per set (phi).
//   * ZL_SLOT_TMP_A / _B are set 0's sort pair under another name: the bases entry points (upload staging, download, generation, the
//     fixed-base and window tables, their batch normalisation) use them as general temporaries, and ZL_SLOT_NTT_VEC (= _B) is the transform's
//     vector between passes.  None of these calls contains an MSM and each has drained when it returns, so no sort is in flight when they
//     resize the blocks (a proof's transforms run on ctx->aux2, whose slots are its own).
//   * ZL_SLOT_STAGING: host scalars / vectors uploaded for one call.  ZL_SLOT_GROTH16: the witness map's vectors (the quotient of the last
//     proof stays there, zl_ctx::g16_h).  ZL_SLOT_TESTHOOK: inputs and outputs of the test hooks.
//   * ZL_SLOT_PAIR_*: the device product of pairings.  ZL_SLOT_PAIR_FEXP: the device final exponentiations (zl_pairing_dev.hip fexp): exponent words, values,
//     flags and the window powers of one launch.  Its own slot: it reads the Miller values of a groups launch out of ZL_SLOT_PAIR_ACC on the same stream.
//   * ZL_SLOT_DECODE_IN / _OUT: the packed records and the decoded points of the device point / proof decoder (zl_decode_dev.hip).  Not the PAIR_* slots:
//     zl_groth16_verify_batch_bytes runs the decoder and the product of pairings in one call.
//   * ZL_SLOT_MSM_MULTI: the slice partials and the result staging of one chunk of zl_msm_multi_dev (zl_msm_multi.hip); the chunks of a call follow
//     each other on ctx->stream.  Its own slot: a caller may hold scalars for it in any other block of the ctx.
//   * ZL_SLOT_G16_BATCH: one chunk of zl_groth16_prove_batch (zl_groth16.hip): the assignments, the witness map's [3][chunk][N] vectors and the three scalar
//     matrices its multi-MSMs read; the transforms in between use ZL_SLOT_NTT_VEC, the multi-MSMs ZL_SLOT_MSM_MULTI, one after the other on ctx->stream.
//   * ZL_SLOT_POSEIDON: the flag word and one staged chunk (inputs, outputs) of the batched Poseidon entry points (zl_poseidon_dev.hip), under a byte budget;
//     the chunks of a call follow each other on ctx->stream.  Its own slot: a caller may hold device operands for the _dev forms in any other block.
//   * ZL_SLOT_EDWARDS: the flag word, the per-lane window tables and one staged chunk of the embedded-curve entry points (zl_edwards_dev.hip), under a byte
//     budget.  Its own slot: the hybrid calls keep the shared secrets of a chunk here while the duplex call underneath stages through ZL_SLOT_POSEIDON.
//     The assignment trace (k_ed_mul_trace) takes NO bytes of it for its kernel: the points it keeps between its passes live in the row's own step cells
//     (8 elements of 48 B in the 416 B of a step).  Only its staged operands count: 64 + 32 B of inputs, and, in the host-pointer form, the row itself
//     (14 bits - 5 elements: 112 736 B at 252 bits, so some 2 300 rows a chunk under the 256 MiB budget) and 64 B for Q.
//     The hybrid-encryption trace (k_ed_hybrid_ladders, then k_pos_duplex_trace_in) likewise: staged operands and, in the host-pointer form, the row (27 bits -
//     13 + 2 T + H + 3 S elements: 247 680 B at 252 bits and (3; 0, 1), some 1 000 rows a chunk); its cipher launch stages nothing and takes no byte of
//     ZL_SLOT_POSEIDON while this slot holds the chunk.
enum zl_slot : int {
    ZL_SLOT_SET0_COUNTS = 0, ZL_SLOT_SET0_ENTRIES = 1, ZL_SLOT_SET0_BUCKETS = 2, ZL_SLOT_SET0_PARTIALS = 3, ZL_SLOT_SET0_TAIL = 4,
    ZL_SLOT_SORT_A = 5, ZL_SLOT_SORT_B = 6,
    ZL_SLOT_TMP_A = ZL_SLOT_SORT_A, ZL_SLOT_TMP_B = ZL_SLOT_SORT_B, ZL_SLOT_NTT_VEC = ZL_SLOT_SORT_B,
    ZL_SLOT_STAGING = 7, ZL_SLOT_GROTH16 = 8, ZL_SLOT_TESTHOOK = 9,
    ZL_SLOT_SET1_COUNTS = 10, ZL_SLOT_SET1_ENTRIES = 11, ZL_SLOT_SET1_BUCKETS = 12, ZL_SLOT_SET1_PARTIALS = 13,
    ZL_SLOT_SET2_COUNTS = 14, ZL_SLOT_SET2_ENTRIES = 15, ZL_SLOT_SET2_BUCKETS = 16, ZL_SLOT_SET2_PARTIALS = 17,
    ZL_SLOT_PHI_ONE_KEY = 18,
    ZL_SLOT_SET1_TAIL = 19,
    ZL_SLOT_SET0_PHI = 20, ZL_SLOT_SET1_PHI = 21, ZL_SLOT_SET2_PHI = 22,
    ZL_SLOT_SET2_TAIL = 23,
    ZL_SLOT_SET1_SORT_A = 24, ZL_SLOT_SET1_SORT_B = 25, ZL_SLOT_SET2_SORT_A = 26, ZL_SLOT_SET2_SORT_B = 27,
    ZL_SLOT_SET3_COUNTS = 28, ZL_SLOT_SET3_ENTRIES = 29, ZL_SLOT_SET3_BUCKETS = 30, ZL_SLOT_SET3_PARTIALS = 31, ZL_SLOT_SET3_TAIL = 32,
    ZL_SLOT_SET3_SORT_A = 33, ZL_SLOT_SET3_SORT_B = 34, ZL_SLOT_SET3_PHI = 35,
    ZL_SLOT_PAIR_IN = 36, ZL_SLOT_PAIR_LINES = 37, ZL_SLOT_PAIR_ACC = 38, ZL_SLOT_PAIR_PREP = 39,
    ZL_SLOT_DECODE_IN = 40, ZL_SLOT_DECODE_OUT = 41,
    ZL_SLOT_MSM_MULTI = 42, ZL_SLOT_G16_BATCH = 43,
    ZL_SLOT_PAIR_FEXP = 44,
    ZL_SLOT_POSEIDON = 45,
    ZL_SLOT_EDWARDS = 46,
    ZL_SLOT_COUNT = 47
};
// the slots of MSM buffer set 0..3; sort_a / sort_b are used by a job that owns its sort (side by side), every other job sorts in set 0's pair
struct zl_msm_set_slots {
    zl_slot data[4], tail, sort_a, sort_b, phi;  // data: counters | sorted entries | buckets | chunk partials
};
constexpr zl_msm_set_slots ZL_MSM_SET[4] = {
    {{ZL_SLOT_SET0_COUNTS, ZL_SLOT_SET0_ENTRIES, ZL_SLOT_SET0_BUCKETS, ZL_SLOT_SET0_PARTIALS}, ZL_SLOT_SET0_TAIL, ZL_SLOT_SORT_A, ZL_SLOT_SORT_B, ZL_SLOT_SET0_PHI},
    {{ZL_SLOT_SET1_COUNTS, ZL_SLOT_SET1_ENTRIES, ZL_SLOT_SET1_BUCKETS, ZL_SLOT_SET1_PARTIALS}, ZL_SLOT_SET1_TAIL, ZL_SLOT_SET1_SORT_A, ZL_SLOT_SET1_SORT_B, ZL_SLOT_SET1_PHI},
    {{ZL_SLOT_SET2_COUNTS, ZL_SLOT_SET2_ENTRIES, ZL_SLOT_SET2_BUCKETS, ZL_SLOT_SET2_PARTIALS}, ZL_SLOT_SET2_TAIL, ZL_SLOT_SET2_SORT_A, ZL_SLOT_SET2_SORT_B, ZL_SLOT_SET2_PHI},
    {{ZL_SLOT_SET3_COUNTS, ZL_SLOT_SET3_ENTRIES, ZL_SLOT_SET3_BUCKETS, ZL_SLOT_SET3_PARTIALS}, ZL_SLOT_SET3_TAIL, ZL_SLOT_SET3_SORT_A, ZL_SLOT_SET3_SORT_B, ZL_SLOT_SET3_PHI},
};
// every slot of the four sets and every slot outside them has one owner (the aliases of set 0's sort pair above are the only sharing)
constexpr bool zl_slots_disjoint() {
    int owners[ZL_SLOT_COUNT] = {};
    for (const zl_msm_set_slots& s : ZL_MSM_SET)
        for (zl_slot x : {s.data[0], s.data[1], s.data[2], s.data[3], s.tail, s.sort_a, s.sort_b, s.phi}) {
            if (x < 0 || x >= ZL_SLOT_COUNT) return false;
            owners[x]++;
        }
    for (zl_slot x : {ZL_SLOT_PHI_ONE_KEY, ZL_SLOT_STAGING, ZL_SLOT_GROTH16, ZL_SLOT_TESTHOOK, ZL_SLOT_PAIR_IN, ZL_SLOT_PAIR_LINES, ZL_SLOT_PAIR_ACC, ZL_SLOT_PAIR_PREP,
                      ZL_SLOT_DECODE_IN, ZL_SLOT_DECODE_OUT, ZL_SLOT_MSM_MULTI, ZL_SLOT_G16_BATCH, ZL_SLOT_PAIR_FEXP, ZL_SLOT_POSEIDON, ZL_SLOT_EDWARDS}) {
        if (x < 0 || x >= ZL_SLOT_COUNT) return false;
        owners[x]++;
    }
    for (int n : owners)
        if (n > 1) return false;
    return true;
}
static_assert(zl_slots_disjoint(), "scratch slots: the four MSM buffer sets, the shared / staging slots, the pairing product and the decoder must not collide");
static_assert(ZL_SLOT_DECODE_IN != ZL_SLOT_PAIR_IN && ZL_SLOT_DECODE_OUT != ZL_SLOT_PAIR_PREP && ZL_SLOT_DECODE_OUT != ZL_SLOT_PAIR_LINES && ZL_SLOT_DECODE_OUT != ZL_SLOT_PAIR_ACC,
              "the decoder keeps its own slots: the bytes-in verifier decodes and pairs in one call");
static_assert(ZL_SLOT_PAIR_FEXP != ZL_SLOT_PAIR_ACC && ZL_SLOT_PAIR_FEXP != ZL_SLOT_PAIR_IN && ZL_SLOT_PAIR_FEXP != ZL_SLOT_PAIR_PREP && ZL_SLOT_PAIR_FEXP != ZL_SLOT_PAIR_LINES &&
                  ZL_SLOT_PAIR_FEXP != ZL_SLOT_DECODE_IN && ZL_SLOT_PAIR_FEXP != ZL_SLOT_DECODE_OUT,
              "the final exponentiations read a groups launch's accumulators in place and run inside the bytes-in verifier: their own slot");
static_assert(ZL_SLOT_EDWARDS != ZL_SLOT_POSEIDON, "a hybrid call holds its shared secrets while the duplex call underneath stages its own chunk");
static_assert(ZL_SLOT_TMP_A == ZL_MSM_SET[0].sort_a && ZL_SLOT_TMP_B == ZL_MSM_SET[0].sort_b && ZL_SLOT_NTT_VEC == ZL_MSM_SET[0].sort_b,
              "the general temporaries and the transform's vector are set 0's sort pair and nothing else (see the map)");
struct zl_twiddles {
    void* d_lo = nullptr;  // w^i, i < 2^lo_bits
    void* d_hi = nullptr;  // w^(i << lo_bits)
    void* d_small = nullptr;  // per-radix tables
    void* d_small_limbs = nullptr;  // the per-radix tables as limbs (read by the lazy passes' butterflies)
    void* d_last = nullptr;   // combined inter-factor twiddles of the last pass, one per element (multi-pass sizes, built on first use)
    void* d_row[4] = {nullptr, nullptr, nullptr, nullptr};  // per-row twiddles of a MIDDLE pass (index: pass - 1), one row per value of the tile's high index; lazy passes only
    size_t last_bytes = 0;    // ... its size, and when it was last used: the tables of one ctx share a byte budget (ZL_TUNE_NTT_LAST_MB), least recently used first out
    uint64_t last_used = 0;
    unsigned lo_bits = 0;
};
struct zl_r1cs_dev {  // device-resident R1CS matrices (CSR; coefficients in Montgomery form)
    void* d_base = nullptr;
    size_t off_ptr[3] = {0, 0, 0}, off_col[3] = {0, 0, 0}, off_val[3] = {0, 0, 0};
    uint32_t n_constraints = 0, n_instance = 0, n_witness = 0;
    size_t nnz[3] = {0, 0, 0};  // non-zeros of A, B, C (the witness map picks the row-parallel product for matrices with long rows)
    int curve = 0;
};
struct zl_ctx {
    // A FORK (zl_ctx_fork) is a second prover lane on the parent's device: its own streams, scratch, events, workers and twiddle tables, and READ access to the
    // parent's device-resident objects (bases with their tables, R1CS matrices) through zl_find_bases / zl_find_r1cs -- so N host threads prove side by side
    // over ONE copy of a proving key, like N threads sharing the reference's `&ProvingContext` (groth16.rs:445-457 takes it by shared reference).
    zl_ctx* parent = nullptr;
    std::atomic<int> forks{0};  // live forks of this ctx: its handles cannot be freed while any exists
    mutable std::shared_mutex maps_mu;  // guards the two handle maps below: lookups from the lanes (shared) against uploads (exclusive); entries are node-stable
    std::vector<zl_ctx*> fork_list;  // the live forks (under maps_mu): a parent destroyed first orphans them (parent = nullptr: their lookups of its handles then fail with ZL_EHANDLE instead of reading freed memory)
    int fork_seq = 0;           // forks number their own handles from (seq << 48) | 1: no value of theirs collides with one of the parent's
    int device = 0;
    int cu_count = 0;                  // compute units of the device (grid of the persistent accumulation kernel)
    hipStream_t stream = nullptr;      // stream in use
    hipStream_t own_stream = nullptr;  // created by the ctx
    int last_hip = 0;
    int msm_c = 0;
    int msm_cover = 0;  // TEST HOOK (zl_test_msm_exact_cover): > 0 plans BLS12-381 G1 MSMs on the exact-cover plan at any size, < 0 never; 0: the picker (zl_msm_job.h)
    int timing_on = 0;
    zl_timing timing{};
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::map<uint64_t, zl_bases> bases;
    std::map<uint64_t, zl_r1cs_dev> r1cs;
    uint64_t next_handle = 1;
    zl_scratch scratch[ZL_SLOT_COUNT];  // by zl_slot: the map above
    std::map<uint64_t, zl_twiddles> twiddles;  // key: curve<<16 | log_n<<1 | inverse
    size_t ntt_last_bytes = 0;   // bytes held by the d_last tables of this ctx
    // events of the job pipelines, created once and reused by every call: a hipEventCreate / hipEventDestroy pair costs ~50 us of host time, and a
    // four-job pipeline used 14 of them per call -- 0.8 ms at the END of every Groth16 proof (round 4 host trace, profiles/r04_g16_share_ab.log)
    std::vector<hipEvent_t> ev_pool[2];  // [0] hipEventDisableTiming, [1] timing
    // A ctx is SINGLE-CALLER (include/zl_backend.h): the pools above, the scratch slots and the streams belong to the one call in flight.  The job pipeline
    // holds this flag while it uses pool events (zl_ctx_events returns a pointer into the vector: a second, concurrent pipeline on the same ctx would alias
    // the events and a growing pool would move them -- ADVICE r4); a second caller gets ZL_EINVAL instead of a race.  Concurrency = one ctx per thread
    // (Groth16 runs its G2 MSM and witness map on ctx->aux / aux2 for that reason).
    std::atomic<int> pipeline_busy{0};
    uint64_t ntt_clock = 0;
    hipStream_t stream_sort = nullptr;  // pipelined MSM batches: sort | accumulate (ctx->stream) | tail
    hipStream_t stream_lane[4] = {nullptr, nullptr, nullptr, nullptr};  // batches of SMALL MSMs: every job runs sort, accumulation and tail on the stream of its buffer set, the jobs side by side
    hipStream_t stream_tail[3] = {nullptr, nullptr, nullptr};  // one tail stream per buffer set: the tails of consecutive small jobs run side by side
    hipStream_t stream_copy = nullptr;  // zl_msm with host scalars: chunked H2D copies that run under the MSMs of the earlier chunks
    void* pinned = nullptr;  // pinned host staging for pipelined results
    size_t pinned_cap = 0;
    zl_ctx* aux2 = nullptr;  // second auxiliary context (Groth16: the witness map runs beside the witness-only MSMs)
    zl_ctx* stream_lane_ctx = nullptr;  // the fork zl_groth16_prove_circuits keeps for its second host thread (zl_ctx_drop_lanes / zl_ctx_destroy release it)
    zl_ctx* aux = nullptr;  // auxiliary stream + scratch set (Groth16: the G2 MSM overlaps the G1 MSMs)
    void* fb_table[4] = {nullptr, nullptr, nullptr, nullptr};  // fixed-base window tables of the generators (per group config, built on first use)
    zl_worker* workers[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // persistent host threads of this ctx: 0 witness-map issue, 1 G2 MSM (Groth16); 2..5 one per lane stream (side-by-side MSM batches)
    void* g16_h = nullptr;  // quotient polynomial of the last zl_groth16_prove (inside ZL_SLOT_GROTH16; reset when the next proof starts)
    size_t g16_h_n = 0;
    int ntt_fit_beside = 0;  // this ctx's transforms run beside a kernel that leaves 96 registers per SIMD (a proof's witness map: ctx->aux2): use the capped passes (zl_ntt.hip)
    void* poseidon_tab[2 * 4] = {};  // Poseidon round keys, MDS entries and the domain tag in Montgomery form, per curve and width ([4 * curve + width - 3], zl_poseidon_dev.hip): each built once by the ROOT ctx, read by its forks, freed at destroy
    void* g16_z = nullptr;  // the canonical assignment of the last witness-map-only run (sharded proofs: the other ranks copy their slices from here)
    // MEASUREMENT ONLY (zl_test_acc_clock): when non-null, large G1 accumulations run as k_msm_accumulate_clk and leave four clock reads per wave here
    void* acc_clk = nullptr;
    size_t acc_clk_cap = 0, acc_clk_waves = 0;
};

// handle lookup: a ctx's own objects first, then its parent's (forks).  The maps of a ctx with live forks are read-only (uploads and frees are refused), so
// concurrent finds from several lanes are plain concurrent reads of a std::map.
inline const zl_bases* zl_find_bases(const zl_ctx* ctx, uint64_t handle) {
    for (const zl_ctx* c = ctx; c; c = c->parent) {
        std::shared_lock<std::shared_mutex> lk(c->maps_mu);
        auto it = c->bases.find(handle);
        if (it != c->bases.end()) return &it->second;
    }
    return nullptr;
}
inline const zl_r1cs_dev* zl_find_r1cs(const zl_ctx* ctx, uint64_t handle) {
    for (const zl_ctx* c = ctx; c; c = c->parent) {
        std::shared_lock<std::shared_mutex> lk(c->maps_mu);
        auto it = c->r1cs.find(handle);
        if (it != c->r1cs.end()) return &it->second;
    }
    return nullptr;
}
// the lazily built per-handle caches (zl_bases::d_endo, first_xy) are filled under this lock: two lanes may meet on the first use of a shared handle
inline std::mutex& zl_bases_cache_mutex() {
    static std::mutex m;
    return m;
}

// the auxiliary contexts of a ctx (Groth16: aux = G2 MSM, aux2 = witness map) and EVERY stream the ctx will ever use, created together in one fixed order (zl_capi.hip)
int zl_ctx_aux_init(zl_ctx* ctx);
int zl_ctx_streams_init(zl_ctx* ctx);

// The fork zl_groth16_prove_circuits keeps for its second host thread is the LIBRARY's, not the caller's: it must not pin the parent's handles once the call
// that used it has returned (zl_bases_free / zl_r1cs_free / zl_bases_precompute on the root ctx returned ZL_EINVAL after one prove_many(),
// and the callers that ignored the code leaked the whole device-resident key).  Every entry that refuses to run beside a live fork releases that idle lane first;
// forks the CALLER made (zl_ctx_fork) still pin the handles, as documented.
inline void zl_ctx_release_idle_lane(zl_ctx* ctx) {
    if (ctx && ctx->stream_lane_ctx && !ctx->pipeline_busy.load()) (void)zl_ctx_drop_lanes(ctx);
}

// developer tuning knob / deployment limit read from the environment (unset = the default)
inline int zl_tune(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}
// How msm_run_jobs_t (zl_msm.hip) runs a batch of `count` >= 2 jobs, the biggest of `biggest` points: `side` = every job on the lane of its buffer set, the jobs
// side by side (else the three-stream pipeline: sort | accumulate | tail over three rotating buffer sets); `lanes` = buffer sets in rotation; `phased` =
// phase-major issue (all sorts, then the accumulations and tails).  The measurements behind the thresholds are with the driver.
struct zl_msm_batch_form {
    bool side;
    size_t lanes;
    bool phased;
};
inline zl_msm_batch_form zl_msm_batch_form_of(size_t count, uint64_t biggest) {
    zl_msm_batch_form f;
    f.side = biggest <= ((uint64_t)1 << zl_tune("ZL_TUNE_SIDE_BY_SIDE_LOG", 20));
    f.lanes = f.side ? std::min<size_t>(count, (size_t)std::min(4, std::max(1, zl_tune("ZL_TUNE_SIDE_LANES", 4)))) : 3;
    f.phased = f.side && count <= f.lanes && biggest >= ((uint64_t)1 << zl_tune("ZL_TUNE_PHASED_MIN_LOG", 17));
    return f;
}
// the first `count` events of the ctx's pool of one kind (grown on demand; owned by the ctx: zl_ctx_destroy).  The pointer is valid until the next call for
// the SAME kind that has to grow the pool: callers take it once per pipeline call, under ctx->pipeline_busy
inline int zl_ctx_events(zl_ctx* ctx, int timing, size_t count, hipEvent_t** out) {
    std::vector<hipEvent_t>& pool = ctx->ev_pool[timing ? 1 : 0];
    while (pool.size() < count) {
        hipEvent_t e = nullptr;
        const hipError_t he = timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming);
        if (he != hipSuccess) { ctx->last_hip = (int)he; return ZL_EHIP; }
        pool.push_back(e);
    }
    *out = pool.data();
    return ZL_OK;
}
inline zl_worker& zl_ctx_worker(zl_ctx* ctx, int k) {
    if (!ctx->workers[k]) ctx->workers[k] = new zl_worker();
    return *ctx->workers[k];
}
// grow-only device scratch slot (growth synchronises ctx->stream only and frees the old block: callers size a slot before anything that uses it is in flight)
inline int zl_scratch_get(zl_ctx* ctx, zl_slot slot, size_t bytes, void** out) {
    zl_scratch& s = ctx->scratch[slot];
    if (s.cap < bytes) {
        if (s.p) {
            hipError_t e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) { ctx->last_hip = (int)e; return ZL_EHIP; }
            (void)hipFree(s.p);
            s.p = nullptr;
            s.cap = 0;
        }
        size_t want = bytes + bytes / 8 + 4096;
        hipError_t e = hipMalloc(&s.p, want);
        if (e != hipSuccess) { ctx->last_hip = (int)e; s.p = nullptr; return ZL_ENOMEM; }
        s.cap = want;
    }
    *out = s.p;
    return ZL_OK;
}

struct zl_test_msm_plan_s;  // (include/zl_backend_test.h)
// entry points implemented per translation unit; the MSM file is compiled once per group (suffix = group config)
#define ZL_DECL_GROUP(G)                                                                                                   \
    int zl_msm_run_##G(zl_ctx* ctx, const zl_bases& b, size_t first, const void* d_scalars, size_t n, uint64_t* out_partial); \
    int zl_msm_run_batch_##G(zl_ctx* ctx, const zl_bases& b, size_t first, const void* const* d_scalars, size_t n, size_t count, uint64_t* out_partials); \
    int zl_msm_run_jobs_##G(zl_ctx* ctx, const zl_bases* const* bases, const size_t* first, const void* const* d_scalars, const size_t* n, const hipEvent_t* wait, size_t count, uint64_t* out_partials, const std::atomic<int>* recorded, const std::function<void(size_t)>* on_done); \
    int zl_partial_to_affine_##G(const uint64_t* partial, uint64_t* out_xy, uint8_t* out_inf);                              \
    int zl_partials_fold_##G(const uint64_t* partials, size_t count, uint64_t* out_partial);                                \
    int zl_partial_from_affine_##G(const uint64_t* xy, uint64_t* out_partial);                                \
    int zl_bases_upload_##G(zl_ctx* ctx, const void* xy, size_t n, size_t stride, long inf_off, unsigned flags, zl_bases* out); \
    int zl_bases_generate_##G(zl_ctx* ctx, const uint64_t* k, size_t n, zl_bases* out);                                     \
    int zl_bases_download_##G(zl_ctx* ctx, const zl_bases& b, size_t first, size_t count, uint64_t* out_xy);                \
    int zl_bases_precompute_##G(zl_ctx* ctx, zl_bases& b, int c);                                                           \
    int zl_msm_plan_report_##G(zl_ctx* ctx, const zl_bases& b, size_t first, size_t n, struct zl_test_msm_plan_s* out);       \
    int zl_msm_multi_run_##G(zl_ctx* ctx, const zl_bases& b, size_t first, const void* d_scalars, size_t n, size_t stride_scalars, size_t count, uint64_t* out_xy, uint8_t* out_inf); \
    int zl_bases_concat_##G(zl_ctx* ctx, const zl_bases* const* parts, const size_t* first, const size_t* n, size_t count, zl_bases* out);
ZL_DECL_GROUP(BlsG1)
ZL_DECL_GROUP(BnG1)
ZL_DECL_GROUP(BlsG2)
ZL_DECL_GROUP(BnG2)
// dispatch on (curve, group)
#define ZL_DISPATCH(curve, group, fn, ...)                                                   \
    (((curve) == ZL_BLS12_381 && (group) == ZL_G1)   ? fn##_BlsG1(__VA_ARGS__)               \
     : ((curve) == ZL_BN254 && (group) == ZL_G1)     ? fn##_BnG1(__VA_ARGS__)                \
     : ((curve) == ZL_BLS12_381 && (group) == ZL_G2) ? fn##_BlsG2(__VA_ARGS__)               \
     : ((curve) == ZL_BN254 && (group) == ZL_G2)     ? fn##_BnG2(__VA_ARGS__)                \
                                                     : (int)ZL_EINVAL)
int zl_ntt_run(zl_ctx* ctx, int curve, void* d_data, unsigned log_n, unsigned flags);
int zl_ntt_run_batch(zl_ctx* ctx, int curve, void* d_data, unsigned log_n, unsigned flags, unsigned count, size_t stride_bytes);  // `count` equal transforms, one launch per pass
int zl_ntt_cross_run(zl_ctx* ctx, int curve, void* d_data, unsigned log_n, unsigned log_g, unsigned rank, unsigned flags);
void zl_ntt_free(zl_ctx* ctx);
