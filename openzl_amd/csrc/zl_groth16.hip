// zl_groth16.hip -- Groth16 prover on the device: QAP witness map (NTT block) + the five MSMs + host assembly.
//
// Replaces ark_groth16::create_random_proof / create_proof_with_assignment + R1CStoQAP::witness_map (ark-groth16 0.3.0)
// behind `Groth16::<E>::prove` (/root/reference/plugins/arkworks/src/groth16.rs:445-457):
//   a_i = <A_i,z>, b_i = <B_i,z>, c_i = <C_i,z>; a[n_constraints + j] = z[j] for the instance block
//   a,b,c <- coset_fft(ifft(.)); ab = (a o b - c) / (g^N - 1); h = coset_ifft(ab)
//   A = r*delta1 + a_query[0] + MSM(a_query[1..], z[1..]) + alpha1      (B1 in G1, B2 in G2 likewise with s, beta)
//   C = s*A + r*B1 - r*s*delta1 + MSM(l_query, z_wit) + MSM(h_query, h[..N-1])
// The R1CS arrives already synthesised (the reference moves a pre-built constraint system into arkworks the same way,
// plugins/arkworks/src/constraint/mod.rs:179-197); sparse mat-vec, pointwise ops and Montgomery entry/exit are small
// elementwise kernels around zl_ntt_run / zl_msm_run; the window Horner and the final few group operations run on host.
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <array>
#include <thread>
#include <vector>
#include <chrono>
#include <stdio.h>
#include <functional>
#include "zl_ctx.h"
#include "zl_poseidon_dev.h"
#include "zl_edwards_dev.h"

template <class FrP>
__global__ void __launch_bounds__(256) k_fr_to_mont(Fp<FrP>* __restrict__ v, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = zl::to_mont(v[i]);
}
template <class FrP>
__global__ void __launch_bounds__(256) k_fr_from_mont(const Fp<FrP>* __restrict__ in, Fp<FrP>* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = zl::from_mont(in[i]);
}
// out[row] = sum_k val[k] * z[col[k]]  (Montgomery); rows >= n_rows: out[n_rows + j] = z[j] for j < tail (A only), else 0.
// blockIdx.y = proof: z of proof v at z_all + v nv, out at out_all + v N (a single proof is a launch with grid.y = 1)
template <class FrP>
__global__ void __launch_bounds__(256) k_r1cs_spmv(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ col, const Fp<FrP>* __restrict__ val,
                                                    const Fp<FrP>* __restrict__ z_all, uint32_t nv, uint32_t n_rows, uint32_t tail, uint32_t N,
                                                    Fp<FrP>* __restrict__ out_all) {
    using F = Fp<FrP>;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const F* z = z_all + (size_t)blockIdx.y * nv;
    F acc = F::zero();
    if (i < n_rows) {
        for (uint32_t k = ptr[i]; k < ptr[i + 1]; k++) acc = zl::add(acc, zl::mul(val[k], z[col[k]]));
    } else if (i - n_rows < tail) {
        acc = z[i - n_rows];
    }
    out_all[(size_t)blockIdx.y * N + i] = acc;
}
// The same product with EIGHT lanes per row (round 6): a row of the Poseidon circuit's A and B holds up to ~150 terms (the linear layers are merged into the rows), and one
// lane per row walks them as a chain of dependent multiply-adds -- 91 + 68 us for the 235 rows of a one-hash proof, on the critical path in front of the h MSM.  Lane j of
// a group takes the terms k = first + j, + 8, ...; the eight partial sums are folded by three xor-shuffle steps (fully reduced Fr: addition is exact in any order).
template <class FrP>
__global__ void __launch_bounds__(256) k_r1cs_spmv8(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ col, const Fp<FrP>* __restrict__ val,
                                                     const Fp<FrP>* __restrict__ z_all, uint32_t nv, uint32_t n_rows, uint32_t tail, uint32_t N,
                                                     Fp<FrP>* __restrict__ out_all) {
    using F = Fp<FrP>;
    const uint32_t gt = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = gt >> 3, j = gt & 7u;
    if (i >= N) return;  // (N is a multiple of 32: whole groups leave together)
    const F* z = z_all + (size_t)blockIdx.y * nv;
    F acc = F::zero();
    if (i < n_rows) {
        const uint32_t e = ptr[i + 1];
        for (uint32_t k = ptr[i] + j; k < e; k += 8) acc = zl::add(acc, zl::mul(val[k], z[col[k]]));
    } else if (j == 0 && i - n_rows < tail) {
        acc = z[i - n_rows];
    }
#pragma unroll
    for (int d = 4; d >= 1; d >>= 1) {
        F o;
#pragma unroll
        for (int w = 0; w < F::N; w++) o.l[w] = (uint32_t)__shfl_xor((int)acc.l[w], d, 8);
        acc = zl::add(acc, o);
    }
    if (j == 0) out_all[(size_t)blockIdx.y * N + i] = acc;
}
// a = (a*b - c) * zinv
template <class FrP>
__global__ void __launch_bounds__(256) k_qap_pointwise(Fp<FrP>* __restrict__ a, const Fp<FrP>* __restrict__ b, const Fp<FrP>* __restrict__ c,
                                                        Fp<FrP> zinv, uint32_t N) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) a[i] = zl::mul(zl::sub(zl::mul(a[i], b[i]), c[i]), zinv);
}

template <class G>
static XYZZ<typename G::F> affine_from_canon(const uint64_t* xy) {
    using F = typename G::F;
    constexpr int WORDS = FieldIO<F>::WORDS;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(xy);
    uint32_t acc = 0;
    for (int k = 0; k < 2 * WORDS; k++) acc |= w[k];
    if (!acc) return XYZZ<F>::inf();
    return XYZZ<F>::from_affine(Affine<F>{FieldIO<F>::load_canon(w), FieldIO<F>::load_canon(w + WORDS)});
}
template <class G>
static void store_canon(uint64_t* out_xy, uint8_t* out_inf, const XYZZ<typename G::F>& p) {
    using F = typename G::F;
    constexpr int WORDS = FieldIO<F>::WORDS;
    uint32_t* w = reinterpret_cast<uint32_t*>(out_xy);
    *out_inf = p.is_inf() ? 1 : 0;
    if (p.is_inf()) { for (int k = 0; k < 2 * WORDS; k++) w[k] = 0; return; }
    const Affine<F> a = zl::to_affine(p);
    FieldIO<F>::store_canon(w, a.x);
    FieldIO<F>::store_canon(w + WORDS, a.y);
}
template <class F>
static XYZZ<F> from_partial(const uint64_t* partial) {
    XYZZ<F> p;
    memcpy(&p, partial, sizeof p);
    return p;
}

// R1CS matrices -> device (CSR, coefficients converted to Montgomery once).  Static per circuit, like the proving key.
template <class FrP>
static int r1cs_upload_t(zl_ctx* ctx, const zl_r1cs* cs, zl_r1cs_dev* out) {
    using Fr = Fp<FrP>;
    const uint32_t nc = cs->n_constraints;
    size_t bytes = 0;
    auto take = [&](size_t b) { size_t o = bytes; bytes += (b + 255) / 256 * 256; return o; };
    size_t nnz[3];
    for (int m = 0; m < 3; m++) {
        nnz[m] = cs->row_ptr[m][nc];
        out->off_ptr[m] = take((size_t)(nc + 1) * 4);
        out->off_col[m] = take(nnz[m] * 4);
        out->off_val[m] = take(nnz[m] * 32);
        out->nnz[m] = nnz[m];
    }
    void* base = nullptr;
    ZL_HIP(ctx, hipMalloc(&base, bytes ? bytes : 256));
    unsigned char* d = reinterpret_cast<unsigned char*>(base);
    hipStream_t st = ctx->stream;
    hipError_t e = hipSuccess;
    for (int m = 0; m < 3 && e == hipSuccess; m++) {
        e = hipMemcpyAsync(d + out->off_ptr[m], cs->row_ptr[m], (size_t)(nc + 1) * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && nnz[m]) {
            e = hipMemcpyAsync(d + out->off_col[m], cs->col[m], nnz[m] * 4, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipMemcpyAsync(d + out->off_val[m], cs->val[m], nnz[m] * 32, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) {
                hipLaunchKernelGGL((k_fr_to_mont<FrP>), dim3((uint32_t)((nnz[m] + 255) / 256)), dim3(256), 0, st, (Fr*)(d + out->off_val[m]), (uint32_t)nnz[m]);
                e = hipGetLastError();
            }
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { ctx->last_hip = (int)e; (void)hipFree(base); return ZL_EHIP; }
    out->d_base = base;
    out->n_constraints = nc;
    out->n_instance = cs->n_instance;
    out->n_witness = cs->n_witness;
    return ZL_OK;
}

// ---- per-key host state (round 6): the proof's fixed-base products and the folded C query ---------------------------------------------------------------
// A proof multiplies four points OF THE KEY by its blinding scalars (r delta1, s delta1, r s delta1, s delta2; the folded form below also s alpha1 and
// r beta1).  As variable-base products they were 256 doublings + 64 additions each (~0.3 ms in G1, ~0.7 ms in G2, one host thread per product); with the
// multiples d 2^(4 w) P, d = 1 .. 15, w = 0 .. 63, of a key point P tabulated once per key (960 affine points, batch-normalised: one inversion), a product is
// at most 64 mixed additions and no doubling: ~30 us in G1, ~100 us in G2.
template <class F>
struct FixedBase {
    std::vector<Affine<F>> tab;  // [64][15]
    XYZZ<F> p = XYZZ<F>::inf();
    bool tabulated = false;      // false: P is the point at infinity, or some small multiple of it is (a point outside the prime-order group): the plain product
    void build(const XYZZ<F>& point) {
        p = point;
        tabulated = false;
        tab.clear();
        if (p.is_inf()) return;
        std::vector<XYZZ<F>> t((size_t)64 * 15);
        XYZZ<F> base = p;
        for (int w = 0; w < 64; w++) {
            XYZZ<F>* row = &t[(size_t)w * 15];
            row[0] = base;
            for (int d = 1; d < 15; d++) {
                row[d] = row[d - 1];
                zl::add_full(row[d], base);
            }
            zl::add_full(base, row[14]);  // 16 base
        }
        for (const XYZZ<F>& e : t) if (e.is_inf()) return;
        // x = X / zz, y = Y / zzz with 1 / zz = (zz / zzz)^2 (zz^3 = zzz^2): one inversion for all the zzz (prefix products)
        const size_t n = t.size();
        std::vector<F> pre(n);
        pre[0] = t[0].zzz;
        for (size_t i = 1; i < n; i++) pre[i] = zl::mul(pre[i - 1], t[i].zzz);
        F run = zl::inv(pre[n - 1]);
        tab.resize(n);
        for (size_t i = n; i-- > 0;) {
            const F izzz = i ? zl::mul(run, pre[i - 1]) : run;
            run = zl::mul(run, t[i].zzz);
            const F iz = zl::mul(t[i].zz, izzz);
            tab[i] = Affine<F>{zl::canon(zl::mul(t[i].x, zl::sqr(iz))), zl::canon(zl::mul(t[i].y, izzz))};
        }
        tabulated = true;
    }
    XYZZ<F> mul(const uint32_t* k) const {  // k: 256 bits, little-endian words
        if (!tabulated) return zl::mul_scalar_w4(p, k);
        XYZZ<F> acc = XYZZ<F>::inf();
        for (int w = 0; w < 64; w++) {
            const uint32_t d = (k[w >> 3] >> ((w & 7) * 4)) & 15u;
            if (d) {
                const Affine<F>& e = tab[(size_t)w * 15 + d - 1];
                zl::add_mixed(acc, e.x, e.y, false);
            }
        }
        return acc;
    }
};
// The folded C query.  C = sum_w z_i L_i + sum h_i H_i + s A + r B1 - r s delta1 with A = alpha1 + sum z_i a_i + r delta1, B1 = beta1 + sum z_i b_i + s delta1, i.e.
//   C = [ sum_w z_i L_i + sum_i (s z_i) a_i + sum_i (r z_i) b_i + sum h_i H_i ]  +  s alpha1 + r beta1 + r s delta1:
// ONE multi-scalar multiplication over the concatenation l | a | b1 | h of the key's queries with the scalars z_w | s z | r z | h (the two scaled copies of z cost one
// Fr product per variable on the device), plus three fixed-base products.  B1 is never formed, the two VARIABLE-base products s A + r B1 (~0.3 ms of host time behind the
// a and b1 MSMs, on the critical path of a small proof) disappear, and a proof issues two G1 pipelines' worth of launches instead of four.  The price is n_variables more
// points through the bucket method (the a query is used twice) and scaled scalars that have lost the witness's zeros and ones -- so only proofs whose MSMs
// are latency, not throughput, take this form (ZL_TUNE_G16_FOLD_LOG_N).  The result is the same group element: the proof bytes do not change (tests/test_groth16.py).
#define ZL_G16_FOLD_LOG_N 14  // domains up to 2^14 fold on both curves (profiles/r06_fold_ab.log: 2^15 is even on BLS12-381 and a loss on BN254, 2^18 a loss of 14 %)
template <class G1, class G2>
struct G16KeyCache {
    using F1 = typename G1::F;
    using F2 = typename G2::F;
    std::vector<uint32_t> key_words;  // alpha1 | beta1 | delta1 | delta2 as handed in: the tables below belong to exactly these
    FixedBase<F1> alpha1, beta1, delta1;
    FixedBase<F2> delta2;
    zl_bases fold;  // l | a | b1 | h
    uint64_t fold_handles[4] = {0, 0, 0, 0};
    size_t fold_nv = 0, fold_nw = 0, fold_nh = 0;
    bool fold_built = false;
    void drop_fold() {
        free_bases(fold);
        fold_built = false;
    }
    // the three extended queries of zl_groth16_prove_batch (g16_batch_queries below): a | delta1 | alpha1, b2 | delta2 | beta2, l | a | b1 | h | alpha1 | beta1 | delta1
    zl_bases bq[3];
    uint64_t bq_handles[5] = {0, 0, 0, 0, 0};
    size_t bq_nv = 0, bq_nw = 0, bq_nh = 0;
    bool bq_built = false;
    static void free_bases(zl_bases& b) {
        if (b.d_pts) (void)hipFree(b.d_pts);
        if (b.d_endo) (void)hipFree(b.d_endo);
        if (b.d_inf) (void)hipFree(b.d_inf);
        b = zl_bases{};
    }
    void drop_batch() {
        for (zl_bases& b : bq) free_bases(b);
        bq_built = false;
    }
    ~G16KeyCache() { drop_fold(); drop_batch(); }
    // a fresh object for the same key: the host tables come along, the device queries stay with this one (for the proofs of another lane that still use them)
    std::shared_ptr<G16KeyCache> fresh_with_tables() const {
        auto fresh = std::make_shared<G16KeyCache>();
        fresh->key_words = key_words;
        fresh->alpha1 = alpha1;
        fresh->beta1 = beta1;
        fresh->delta1 = delta1;
        fresh->delta2 = delta2;
        return fresh;
    }
};
template <class G1, class G2>
static std::vector<uint32_t> g16_key_words(const zl_g16_pk* pk) {
    constexpr size_t W1 = 2 * FieldIO<typename G1::F>::WORDS, W2 = 2 * FieldIO<typename G2::F>::WORDS;
    std::vector<uint32_t> w(3 * W1 + W2);
    memcpy(&w[0], pk->alpha_g1, W1 * 4);
    memcpy(&w[W1], pk->beta_g1, W1 * 4);
    memcpy(&w[2 * W1], pk->delta_g1, W1 * 4);
    memcpy(&w[3 * W1], pk->delta_g2, W2 * 4);
    return w;
}
// the cache of this key (built on first use), with the folded query for (nv, nw, nh) if `want_fold`.  bs: a, b1, h, l handles of the key
template <class G1, class G2>
static int g16_key_cache(zl_ctx* ctx, const zl_g16_pk* pk, const zl_bases* const* bs, bool want_fold, size_t nv, size_t nw, size_t nh,
                         std::shared_ptr<G16KeyCache<G1, G2>>* out) {
    using KC = G16KeyCache<G1, G2>;
    const std::vector<uint32_t> words = g16_key_words<G1, G2>(pk);
    const uint64_t hs[4] = {pk->l_query, pk->a_query, pk->b_g1_query, pk->h_query};
    std::lock_guard<std::mutex> lk(zl_bases_cache_mutex());  // (two lanes may prove over one key for the first time together)
    std::shared_ptr<KC> kc = std::static_pointer_cast<KC>(bs[3]->g16_cache);
    if (!kc || kc->key_words != words) {
        kc = std::make_shared<KC>();
        kc->key_words = words;
        kc->alpha1.build(affine_from_canon<G1>(pk->alpha_g1));
        kc->beta1.build(affine_from_canon<G1>(pk->beta_g1));
        kc->delta1.build(affine_from_canon<G1>(pk->delta_g1));
        kc->delta2.build(affine_from_canon<G2>(pk->delta_g2));
        bs[3]->g16_cache = kc;
    }
    if (want_fold && !(kc->fold_built && kc->fold_nv == nv && kc->fold_nw == nw && kc->fold_nh == nh && !memcmp(kc->fold_handles, hs, sizeof hs))) {
        if (kc.use_count() > 2) {  // a proof on another lane still works with the old folded query: a fresh cache object takes its place
            kc = kc->fresh_with_tables();
            bs[3]->g16_cache = kc;
        }
        kc->drop_fold();
        const zl_bases* parts[4] = {bs[3], bs[0], bs[1], bs[2]};
        const size_t first[4] = {0, 0, 0, 0}, n[4] = {nw, nv, nv, nh};
        zl_bases f;
        const int rc = ZL_DISPATCH(pk->curve, ZL_G1, zl_bases_concat, ctx, parts, first, n, 4, &f);
        if (rc) return rc;
        f.curve = (int)pk->curve;
        f.group = ZL_G1;
        kc->fold = f;
        memcpy(kc->fold_handles, hs, sizeof hs);
        kc->fold_nv = nv;
        kc->fold_nw = nw;
        kc->fold_nh = nh;
        kc->fold_built = true;
    }
    *out = kc;
    return ZL_OK;
}
// the scalars of the folded C query: out_zw = z[ni ..) (canonical), out_sz = s z, out_rz = r z (zm: z in Montgomery form, s and r canonical: the Montgomery product of
// z R and s is z s, canonical)
template <class FrP>
__global__ void __launch_bounds__(256) k_g16_fold_scalars(const Fp<FrP>* __restrict__ zc, const Fp<FrP>* __restrict__ zm, Fp<FrP> s, Fp<FrP> r, uint32_t ni, uint32_t nv,
                                                          Fp<FrP>* __restrict__ out_zw, Fp<FrP>* __restrict__ out_sz, Fp<FrP>* __restrict__ out_rz) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const Fp<FrP> m = zm[i];
    out_sz[i] = i ? zl::mul(m, s) : s;  // (variable 0 is the constant ONE: its terms a_0, b_0 enter A and B1 unscaled, whatever the caller wrote there)
    out_rz[i] = i ? zl::mul(m, r) : r;
    if (i >= ni) out_zw[i - ni] = zc[i];
}

// ---- the checks every prover shares ----------------------------------------------------------------------------------------------------------------------
// what a circuit's sizes make of a proof: nv variables (ni instance incl. the constant ONE, nw witness), domain N = 2^log_n >= nc + ni
struct G16Shape {
    uint32_t nc, ni, nw, nv;
    unsigned log_n;
    uint32_t N;
};
template <class FrP>
static int g16_shape(const zl_r1cs_dev* cs, G16Shape* out) {
    const uint32_t nc = cs->n_constraints, ni = cs->n_instance, nw = cs->n_witness;
    const uint64_t nv64 = (uint64_t)ni + nw;
    if (ni < 1 || nv64 >= (1ull << 31)) return ZL_EINVAL;
    unsigned log_n = 1;
    while ((1ull << log_n) < (uint64_t)nc + ni) log_n++;
    if (log_n > (unsigned)FrP::TWO_ADICITY || log_n > 28) return ZL_EINVAL;
    *out = G16Shape{nc, ni, nw, (uint32_t)nv64, log_n, 1u << log_n};
    return ZL_OK;
}
// the key's five queries, bs = a, b1, h, l (G1), b2 (G2): found (a fork reads its parent's key), of the key's curve and their group, long enough for the shape
static int g16_key_handles(const zl_ctx* ctx, const zl_g16_pk* pk, const G16Shape& sh, const zl_bases** bs) {
    const uint64_t hs[5] = {pk->a_query, pk->b_g1_query, pk->h_query, pk->l_query, pk->b_g2_query};
    for (int i = 0; i < 5; i++) {
        bs[i] = zl_find_bases(ctx, hs[i]);
        if (!bs[i] || bs[i]->curve != (int)pk->curve || bs[i]->group != (i == 4 ? ZL_G2 : ZL_G1)) return ZL_EHANDLE;
    }
    if (bs[0]->n < sh.nv || bs[1]->n < sh.nv || bs[4]->n < sh.nv || bs[2]->n < (size_t)sh.N - 1 || bs[3]->n < sh.nw) return ZL_EINVAL;
    return ZL_OK;
}
// The blinding-scalar contract of every prover: r[j], s[j] (4 u64 words each) are below the scalar field's modulus.  A scalar at or above it is not one value
// here: the fixed-base tables walk its 256 bits as they stand, to_mont / mul take reduced operands only (g16_rs, k_g16_fold_scalars, k_g16_batch_scalars), and
// the multi-MSMs of a device batch refuse high bits -- so the paths would disagree.  A plain word comparison (the verifier's, zl_verify.hip: publics_canonical).
template <class FrP>
static bool g16_scalars_canonical(const uint64_t* v, size_t n) {
    static_assert(FrP::N == 8, "scalar fields are 8 x 32 bits");
    for (size_t i = 0; i < n; i++) {
        const uint64_t* w = v + 4 * i;
        uint64_t br = 0;
        for (int j = 0; j < 8; j++) br = (((w[j / 2] >> (32 * (j % 2))) & 0xffffffffu) - FrP::mod(j) - br) >> 63;
        if (!br) return false;  // no borrow out of w - modulus: w >= modulus
    }
    return true;
}
static int g16_blinding_ok(zl_curve_t curve, const uint64_t* r, const uint64_t* s, size_t count) {
    if (count == 0) return ZL_OK;
    if (curve == ZL_BLS12_381) return g16_scalars_canonical<BLS12_381_Fr>(r, count) && g16_scalars_canonical<BLS12_381_Fr>(s, count) ? ZL_OK : ZL_EINVAL;
    if (curve == ZL_BN254) return g16_scalars_canonical<BN254_Fr>(r, count) && g16_scalars_canonical<BN254_Fr>(s, count) ? ZL_OK : ZL_EINVAL;
    return ZL_EINVAL;
}
// what every entry point asks of (pk, r1cs handle, blinding scalars) after its own argument checks, before any device work or thread start: the key's five
// points are there, the circuit is resident and of the key's curve, and all `count` pairs (r[j], s[j]) are canonical -- one bad pair refuses the whole call
static int g16_entry(const zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, const uint64_t* r, const uint64_t* s, size_t count, const zl_r1cs_dev** rd_out) {
    if (!pk->alpha_g1 || !pk->beta_g1 || !pk->delta_g1 || !pk->beta_g2 || !pk->delta_g2) return ZL_EINVAL;
    const zl_r1cs_dev* rd = zl_find_r1cs(ctx, r1cs_handle);
    if (!rd || rd->curve != (int)pk->curve) return ZL_EHANDLE;
    const int rc = g16_blinding_ok(pk->curve, r, s, count);
    if (rc) return rc;
    *rd_out = rd;
    return ZL_OK;
}

// ---- the witness map: z -> h, for one proof or a chunk of them ---------------------------------------------------------------------------------------------
// z arrived in one form (ZL_MONT: Montgomery at d_zm, else canonical at d_zc); the other one is made on the device.  n elements, on ctx->stream
template <class FrP>
static int g16_z_forms(zl_ctx* ctx, Fp<FrP>* d_zc, Fp<FrP>* d_zm, uint32_t n, unsigned flags) {
    hipStream_t st = ctx->stream;
    if (flags & ZL_MONT) {  // arkworks' in-memory assignment: Montgomery limbs; the canonical copy (MSM scalars) is made on the device
        hipLaunchKernelGGL((k_fr_from_mont<FrP>), dim3((n + 255) / 256), dim3(256), 0, st, d_zm, d_zc, n);
    } else {
        ZL_HIP(ctx, hipMemcpyAsync(d_zm, d_zc, (size_t)n * 32, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL((k_fr_to_mont<FrP>), dim3((n + 255) / 256), dim3(256), 0, st, d_zm, n);
    }
    return ZL_OK;
}
// 1 / (g^N - 1): the vanishing polynomial of the domain is constant on the coset g H
template <class FrP>
static Fp<FrP> g16_zinv(unsigned log_n) {
    using Fr = Fp<FrP>;
    Fr gN;
    for (int i = 0; i < Fr::N; i++) gN.l[i] = FrP::generator(i);
    for (unsigned i = 0; i < log_n; i++) gN = zl::sqr(gN);
    return zl::inv(zl::sub(gN, Fr::one()));
}
// `nvec` vectors of 2^log_n elements, one after the other, through the transform steps `steps`: step by step with all vectors in one launch per pass, or
// vector by vector, each through all its steps
static int g16_transform(zl_ctx* ctx, int curve, unsigned char* d, unsigned nvec, unsigned log_n, std::initializer_list<unsigned> steps, bool batched) {
    const size_t stride = (size_t)32 << log_n;
    int rc;
    if (batched && nvec > 1) {
        for (unsigned flags : steps)
            if ((rc = zl_ntt_run_batch(ctx, curve, d, log_n, flags, nvec, stride))) return rc;
        return ZL_OK;
    }
    for (unsigned v = 0; v < nvec; v++)
        for (unsigned flags : steps)
            if ((rc = zl_ntt_run(ctx, curve, d + v * stride, log_n, flags))) return rc;
    return ZL_OK;
}
// spmv, 3 x (ifft, coset fft), pointwise, coset ifft, issued on ctx->stream: z of proof v (Montgomery) at d_zm + v nv, a | b | c laid out [3][count][N] at d_abc;
// leaves h of proof v, in Montgomery form, at d_abc + v N
template <class FrP>
static int g16_witness_map(zl_ctx* ctx, int curve, const zl_r1cs_dev* cs, const Fp<FrP>* d_zm, uint32_t nv, uint32_t count, Fp<FrP>* d_abc, unsigned log_n) {
    using Fr = Fp<FrP>;
    const uint32_t nc = cs->n_constraints, ni = cs->n_instance, N = 1u << log_n, tot = count * N;
    const unsigned char* dm = reinterpret_cast<const unsigned char*>(cs->d_base);
    hipStream_t st = ctx->stream;
    for (int m = 0; m < 3; m++) {
        const uint32_t* ptr = (const uint32_t*)(dm + cs->off_ptr[m]);
        const uint32_t* col = (const uint32_t*)(dm + cs->off_col[m]);
        const Fr* val = (const Fr*)(dm + cs->off_val[m]);
        Fr* out = d_abc + (size_t)m * tot;
        // rows of >= 4 terms on average (A and B of the Poseidon circuit: ~13): eight lanes per row; C (one term per row): one lane
        if (cs->nnz[m] >= (size_t)4 * nc && zl_tune("ZL_TUNE_SPMV8", 1))
            hipLaunchKernelGGL((k_r1cs_spmv8<FrP>), dim3((uint32_t)(((uint64_t)N * 8 + 255) / 256), count), dim3(256), 0, st, ptr, col, val, d_zm, nv, nc, m == 0 ? ni : 0u, N, out);
        else
            hipLaunchKernelGGL((k_r1cs_spmv<FrP>), dim3((N + 255) / 256, count), dim3(256), 0, st, ptr, col, val, d_zm, nv, nc, m == 0 ? ni : 0u, N, out);
    }
    ZL_HIP(ctx, hipGetLastError());
    // a, b, c go through their inverse transform and their coset transform together (one launch per pass, grid.y = vector): a transform of <= 2^16 elements
    // is a chain of passes of ~20 us each whatever its size (16 workgroups at 2^14), so six of a proof's seven transforms cost the latency of two
    // (interleaved A/B, profiles/r06_ntt_batch_ab.log: 1 882 constraints 1.00 -> 0.86 ms, 14 977: 1.58 -> 1.45 (BN254 1.25 -> 1.10), 2^16 - 2^18: -2 %; at 2^20 the passes fill
    // the machine and three at a time is 1-2 % SLOWER beside the G2 accumulation: a single proof's go together on domains up to 2^18 only)
    const bool batched = count > 1 || log_n <= (unsigned)zl_tune("ZL_TUNE_NTT_BATCH_LOG_N", 18);
    unsigned char* d = reinterpret_cast<unsigned char*>(d_abc);
    int rc;
    if ((rc = g16_transform(ctx, curve, d, 3 * count, log_n, {ZL_MONT | ZL_INVERSE, ZL_MONT | ZL_COSET}, batched))) return rc;
    hipLaunchKernelGGL((k_qap_pointwise<FrP>), dim3((tot + 255) / 256), dim3(256), 0, st, d_abc, d_abc + (size_t)tot, d_abc + 2 * (size_t)tot, g16_zinv<FrP>(log_n), tot);
    ZL_HIP(ctx, hipGetLastError());
    return g16_transform(ctx, curve, d, count, log_n, {ZL_MONT | ZL_INVERSE | ZL_COSET}, batched);
}

// ---- one proof on one device (zl_groth16_prove_resident) -------------------------------------------------------------------------------------------------------
static bool g16_host_trace() {
    static const bool on = getenv("ZL_HOST_TRACE") != nullptr;  // developer aid: host-side phase times on stderr
    return on;
}
// (r s) as words, from the product in Fr: (r s) delta1 is then a fixed-base product of its own, independent of the other ones
template <class FrP>
static void g16_rs(const uint32_t* rw, const uint32_t* sw, uint32_t* rsw) {
    Fp<FrP> rm, sm;
    memcpy(rm.l, rw, 32);
    memcpy(sm.l, sw, 32);
    const Fp<FrP> rs = zl::from_mont(zl::mul(zl::to_mont(rm), zl::to_mont(sm)));
    memcpy(rsw, rs.l, 32);
}
// A, B1 and B are one sum each: blinding product + first query point (index 0 pairs with z_0 = 1; null when the MSM started at index 0) + MSM + key point
template <class G>
static XYZZ<typename G::F> g16_blinded_sum(const XYZZ<typename G::F>& blind, const uint64_t* first_xy, const XYZZ<typename G::F>& msm, const uint64_t* key_xy) {
    XYZZ<typename G::F> p = blind;
    if (first_xy) zl::add_full(p, affine_from_canon<G>(first_xy));
    zl::add_full(p, msm);
    zl::add_full(p, affine_from_canon<G>(key_xy));
    return p;
}
// What the phases of a proof share.  It lives in the frame of the prover that runs them; the worker threads, the completion callback and the host threads get a
// pointer to it, and every return of that prover first waits for all of them.
template <class G1, class G2>
struct G16Proof {
    using Fr = Fp<typename G1::FrP>;
    using F1 = typename G1::F;
    using F2 = typename G2::F;
    zl_ctx* ctx;
    const zl_g16_pk* pk;
    const zl_r1cs_dev* cs;
    G16Shape sh;
    const std::chrono::steady_clock::time_point tp0 = std::chrono::steady_clock::now();
    // stage: device pointers into ZL_SLOT_GROTH16, the two events of the witness-map stream, the caller's timing switch
    Fr *d_zc = nullptr, *d_zm = nullptr, *d_abc = nullptr, *d_h = nullptr;
    bool fold = false;     // C from ONE folded query (G16KeyCache): its scalars z_w | s z | r z | h are one vector at d_h - fold_head
    size_t fold_head = 0;
    hipEvent_t ev_z = nullptr, ev_h = nullptr;
    int timing_saved = 0;
    // witness-map job: 4 once ev_h is recorded (the h job of the G1 pipeline, told by `recorded`, may then wait for it), negative on failure
    std::atomic<int> h_recorded{0};
    int rc_wm = ZL_OK;
    // key: handles, first points of the a / b1 / b2 queries, host tables
    const zl_bases* bs[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    uint64_t a0_xy[12], b0_xy[12], b20_xy[24];
    std::shared_ptr<G16KeyCache<G1, G2>> kc;
    // blinding scalars as words and their fixed-base products (threads pre, pre_g2)
    uint32_t rw[8], sw[8], rsw[8];
    std::thread pre, pre_g2;
    XYZZ<F1> r_delta1, s_delta1, rs_delta, c_fixed;
    XYZZ<F2> s_delta2;
    // MSM partial sums where the pipelines put them, and what the G2 worker and the completion callback make of them
    uint64_t g1_sums[4][ZL_PARTIAL_WORDS], g2_sum[ZL_PARTIAL_WORDS];
    int rc_g2 = ZL_OK;
    XYZZ<F1> g_c = XYZZ<F1>::inf();
    bool have_c = false;
    uint64_t a_words[12] = {0}, b_words[24] = {0};
    uint8_t a_inf = 0, b_inf = 0;

    G16Proof(zl_ctx* c, const zl_g16_pk* k, const zl_r1cs_dev* r1cs, const G16Shape& shape) : ctx(c), pk(k), cs(r1cs), sh(shape) {}
    void lap(const char* what) const {
        if (g16_host_trace()) fprintf(stderr, "[zl_groth16 nc=%u] %-28s at %8.1f us\n", (unsigned)sh.nc, what,
                                      (double)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - tp0).count() / 1e3);
    }
    // nothing of the witness map is in flight any more (its issuing thread works on this object): before every return after g16_issue_witness_map
    hipError_t join_witness_map() {
        zl_ctx_worker(ctx, 0).wait();
        return hipStreamSynchronize(ctx->aux2->stream);
    }
};

// Scratch layout and upload: z in both forms on the device, the folded form's scaled copies, ev_z recorded behind them on ctx->stream; the inner calls' timing off.
// `witness` (optional): the assignment arrives in two pieces, `assignment` = the instance block and `witness` = the witness block, as the
// compiler holds them (openzl::Groth16::prove): two copies to the device instead of a host-side concatenation of tens of megabytes per proof
template <class G1, class G2>
static int g16_stage(G16Proof<G1, G2>* p, const uint64_t* assignment, const uint64_t* witness, unsigned flags, const uint64_t* r, const uint64_t* s, bool fold,
                     int ntt_fit_beside) {
    using FrP = typename G1::FrP;
    using Fr = Fp<FrP>;
    zl_ctx* ctx = p->ctx;
    const uint32_t ni = p->sh.ni, nw = p->sh.nw, nv = p->sh.nv, N = p->sh.N;
    hipStream_t st = ctx->stream;
    ctx->g16_h = nullptr;  // the quotient of an earlier proof may live in a scratch block this call re-allocates
    ctx->g16_h_n = 0;
    if (ctx->timing_on) ZL_HIP(ctx, hipEventRecord(ctx->ev[0], st));
    memcpy(p->rw, r, 32);
    memcpy(p->sw, s, 32);
    // z canonical | z Montgomery | a | b | c | [z_w | s z | r z |] h (N entries written, N - 1 used)
    p->fold = fold;
    p->fold_head = fold ? (size_t)nw + 2 * (size_t)nv : 0;
    size_t bytes = 0;
    auto take = [&](size_t b) { size_t o = bytes; bytes += (b + 255) / 256 * 256; return o; };
    const size_t off_zc = take((size_t)nv * 32), off_zm = take((size_t)nv * 32), off_abc = take((size_t)3 * N * 32), off_h = take((p->fold_head + N) * 32) + p->fold_head * 32;
    void* base;
    int rc;
    if ((rc = zl_scratch_get(ctx, ZL_SLOT_GROTH16, bytes, &base))) return rc;
    unsigned char* d = reinterpret_cast<unsigned char*>(base);
    p->d_zc = (Fr*)(d + off_zc);
    p->d_zm = (Fr*)(d + off_zm);
    p->d_abc = (Fr*)(d + off_abc);
    p->d_h = (Fr*)(d + off_h);
    Fr* d_in = (flags & ZL_MONT) ? p->d_zm : p->d_zc;
    if (!witness) {
        ZL_HIP(ctx, hipMemcpyAsync(d_in, assignment, (size_t)nv * 32, hipMemcpyHostToDevice, st));
    } else {
        ZL_HIP(ctx, hipMemcpyAsync(d_in, assignment, (size_t)ni * 32, hipMemcpyHostToDevice, st));
        if (nw) ZL_HIP(ctx, hipMemcpyAsync(d_in + ni, witness, (size_t)nw * 32, hipMemcpyHostToDevice, st));
    }
    if ((rc = g16_z_forms<FrP>(ctx, p->d_zc, p->d_zm, nv, flags))) return rc;
    if (fold) {
        Fr sf, rf;
        memcpy(sf.l, s, 32);
        memcpy(rf.l, r, 32);
        Fr* d_fold = p->d_h - p->fold_head;
        hipLaunchKernelGGL((k_g16_fold_scalars<FrP>), dim3((nv + 255) / 256), dim3(256), 0, st, p->d_zc, p->d_zm, sf, rf, ni, nv, d_fold, d_fold + nw, d_fold + nw + nv);
    }
    // The witness map runs on its own context / stream: it only needs z, like four of the five MSMs, so it runs beside them (memory- and latency-bound kernels
    // in the shadow of the bucket accumulation) behind ev_z; the h MSM waits for ev_h inside the pipeline.
    if ((rc = zl_ctx_aux_init(ctx))) return rc;
    zl_ctx* wm = ctx->aux2;
    wm->ntt_fit_beside = ntt_fit_beside;  // the witness map of a whole proof runs beside the G2 accumulation; on its own (sharded proofs) it takes the faster passes
    p->ev_z = wm->ev[0];
    p->ev_h = wm->ev[1];
    ZL_HIP(ctx, hipEventRecord(p->ev_z, st));
    p->timing_saved = ctx->timing_on;
    ctx->timing_on = 0;  // inner calls must not sync / overwrite the prover's events
    wm->timing_on = 0;
    return ZL_OK;
}
// The ~16 launches of the witness map are issued by a persistent thread of the ctx (worker 0) while the caller goes on to the MSMs (0.15 ms of host
// time that stood in front of every MSM of a small proof): h, canonical, at d_h, ev_h recorded behind it
template <class G1, class G2>
static void g16_issue_witness_map(G16Proof<G1, G2>* p) {
    using FrP = typename G1::FrP;
    zl_ctx_worker(p->ctx, 0).run([p]() {
        auto fail = [&](int code) { p->rc_wm = code; p->h_recorded.store(-1, std::memory_order_release); };
        zl_ctx* wm = p->ctx->aux2;
        const uint32_t N = p->sh.N;
        if (hipSetDevice(p->ctx->device) != hipSuccess || hipStreamWaitEvent(wm->stream, p->ev_z, 0) != hipSuccess) return fail(ZL_EHIP);
        const int rc = g16_witness_map<FrP>(wm, p->pk->curve, p->cs, p->d_zm, p->sh.nv, 1, p->d_abc, p->sh.log_n);
        if (rc) return fail(rc);
        hipLaunchKernelGGL((k_fr_from_mont<FrP>), dim3((N + 255) / 256), dim3(256), 0, wm->stream, p->d_abc, p->d_h, N);
        if (hipGetLastError() != hipSuccess || hipEventRecord(p->ev_h, wm->stream) != hipSuccess) return fail(ZL_EHIP);
        p->h_recorded.store(4, std::memory_order_release);
    });
}
// first points of the a / b queries (index 0 pairs with z[0] = 1): static per key, fetched from the device on the first proof only -- here, before the MSM
// streams are busy (the download uses the ctx's own stream and sort scratch)
template <class G1, class G2>
static int g16_first_points(G16Proof<G1, G2>* p) {
    const struct { const zl_bases* b; int group; uint64_t* out; size_t words; } firsts[3] = {
        {p->bs[0], ZL_G1, p->a0_xy, 12}, {p->bs[1], ZL_G1, p->b0_xy, 12}, {p->bs[4], ZL_G2, p->b20_xy, 24}};
    std::lock_guard<std::mutex> cache_lk(zl_bases_cache_mutex());  // (two lanes may prove over one key for the first time together)
    for (const auto& f : firsts) {
        if (f.b->first_xy.empty()) {
            uint64_t tmp[24] = {0};
            const int rc = ZL_DISPATCH(p->pk->curve, f.group, zl_bases_download, p->ctx, *f.b, 0, 1, tmp);
            if (rc) return rc;
            f.b->first_xy.assign(tmp, tmp + f.words);
        }
        memcpy(f.out, f.b->first_xy.data(), f.words * 8);
    }
    return ZL_OK;
}
// host work that does not depend on the MSMs -- the fixed-base products r delta1, s delta2 and (folded form) s alpha1 + r beta1 + r s delta1, or (four-MSM form)
// s delta1 and -r s delta1 -- runs on two threads while the device is busy: at most 64 mixed additions each from the key's tables
template <class G1, class G2>
static void g16_start_fixed_base(G16Proof<G1, G2>* p) {
    g16_rs<typename G1::FrP>(p->rw, p->sw, p->rsw);
    p->pre = std::thread([p]() {
        const G16KeyCache<G1, G2>& kc = *p->kc;
        p->r_delta1 = kc.delta1.mul(p->rw);
        p->lap("r delta1 done");
        p->rs_delta = kc.delta1.mul(p->rsw);
        if (p->fold) {
            p->c_fixed = kc.alpha1.mul(p->sw);
            zl::add_full(p->c_fixed, kc.beta1.mul(p->rw));
            zl::add_full(p->c_fixed, p->rs_delta);
        } else {
            zl::neg_inplace(p->rs_delta);
            p->s_delta1 = kc.delta1.mul(p->sw);
        }
        p->lap("G1 fixed-base products done");
    });
    p->pre_g2 = std::thread([p]() { p->s_delta2 = p->kc->delta2.mul(p->sw); p->lap("s delta2 done"); });
}
// The G2 MSM runs on an auxiliary stream with its own scratch, issued by worker 1, while the G1 MSMs run on the main streams: the two fill each other's gaps
// (54 -> ~35 ms at 2^20).  Nobody waits for z on the host: the G2 stream waits for ev_z like the witness map.
// (Tried: every MSM of a folded proof behind the witness map, so that the accumulations do not sit on the SIMDs its short passes need -- slower at every size, 235 constraints
// 0.67 -> 0.74, 14 977: 1.58 -> 1.61 (profiles/r06_gate_ab.log): a 2^14 transform is two passes of ~20 us on 16 workgroups whether or not the machine is busy.  What helped
// is running a, b, c through each transform in one launch, g16_witness_map.)
template <class G1, class G2>
static void g16_issue_g2(G16Proof<G1, G2>* p) {
    zl_ctx_worker(p->ctx, 1).run([p]() {
        zl_ctx* aux = p->ctx->aux;
        if (hipSetDevice(aux->device) != hipSuccess || hipStreamWaitEvent(aux->stream, p->ev_z, 0) != hipSuccess) { p->rc_g2 = ZL_EHIP; return; }
        p->rc_g2 = ZL_DISPATCH(p->pk->curve, ZL_G2, zl_msm_run, aux, *p->bs[4], 1, reinterpret_cast<const unsigned char*>(p->d_zc) + 32, p->sh.nv - 1, p->g2_sum);
        if (p->rc_g2 != ZL_OK) return;
        // B = beta2 + sum z_i b2_i + s delta2 is complete here: assembled and normalised (the Fq2 inversion) on this thread, beside the G1 pipeline
        p->pre_g2.join();
        store_canon<G2>(p->b_words, &p->b_inf, g16_blinded_sum<G2>(p->s_delta2, p->b20_xy, from_partial<typename G2::F>(p->g2_sum), p->pk->beta_g2));
        p->lap("B done");
    });
}
// The G1 pipeline, folded form: the a MSM (for A) and ONE MSM over l | a | b1 | h for all of C's sums; the second waits for the witness map's event.
// All its streams start behind an event the pipeline records on ctx->stream (zl_msm.hip: ev_begin), so behind z.
template <class G1, class G2>
static int g16_run_g1_folded(G16Proof<G1, G2>* p) {
    using F1 = typename G1::F;
    const unsigned char* zc = reinterpret_cast<const unsigned char*>(p->d_zc);
    const zl_bases* jb[2] = {p->bs[0], &p->kc->fold};
    const size_t jf[2] = {1, 0};
    const void* js[2] = {zc + 32, p->d_h - p->fold_head};
    const size_t jn[2] = {(size_t)p->sh.nv - 1, p->fold_head + (size_t)p->sh.N - 1};
    const hipEvent_t jw[2] = {nullptr, p->ev_h};
    const std::function<void(size_t)> on_done = [p](size_t i) {
        if (i != 0) return;
        p->pre.join();
        const XYZZ<F1> g_a = g16_blinded_sum<G1>(p->r_delta1, p->a0_xy, from_partial<F1>(p->g1_sums[0]), p->pk->alpha_g1);
        store_canon<G1>(p->a_words, &p->a_inf, g_a);  // A is final: its normalisation (one inversion) runs under the second MSM
        p->g_c = p->c_fixed;
        p->have_c = true;
        p->lap("A done");
    };
    return ZL_DISPATCH(p->pk->curve, ZL_G1, zl_msm_run_jobs, p->ctx, jb, jf, js, jn, jw, 2, &p->g1_sums[0][0], (const std::atomic<int>*)&p->h_recorded, &on_done);
}
// The G1 pipeline, four-MSM form (sort | accumulate | tail of consecutive MSMs overlap, zl_msm.hip): a, b1, l need only z; the h job waits for the witness map's
// event.  Order a, b1, l, h: A and B1 are complete after the first two jobs, and their products s A and r B1 (256 doublings + 64 additions each on the host) run
// on the pipeline's completion thread and one more while the l, h and G2 MSMs are still on the device
template <class G1, class G2>
static int g16_run_g1_four(G16Proof<G1, G2>* p) {
    using F1 = typename G1::F;
    const unsigned char* zc = reinterpret_cast<const unsigned char*>(p->d_zc);
    const size_t nv = p->sh.nv;
    const zl_bases* jb[4] = {p->bs[0], p->bs[1], p->bs[3], p->bs[2]};
    const size_t jf[4] = {1, 1, 0, 0};
    const void* js[4] = {zc + 32, zc + 32, zc + (size_t)p->sh.ni * 32, p->d_h};
    const size_t jn[4] = {nv - 1, nv - 1, (size_t)p->sh.nw, (size_t)p->sh.N - 1};
    const hipEvent_t jw[4] = {nullptr, nullptr, nullptr, p->ev_h};
    const std::function<void(size_t)> on_done = [p](size_t i) {
        if (i != 1) return;
        p->lap("a, b1 delivered");
        p->pre.join();
        const XYZZ<F1> g_a = g16_blinded_sum<G1>(p->r_delta1, p->a0_xy, from_partial<F1>(p->g1_sums[0]), p->pk->alpha_g1);
        const XYZZ<F1> g1_b = g16_blinded_sum<G1>(p->s_delta1, p->b0_xy, from_partial<F1>(p->g1_sums[1]), p->pk->beta_g1);
        p->lap("a, b1 in: s A + r B1 starts");
        {   // s A + r B1 as two single-scalar products side by side (0.3 ms) instead of one interleaved double-scalar product (0.45 ms)
            XYZZ<F1> rb = XYZZ<F1>::inf();
            std::thread t_rb([&]() { rb = zl::mul_scalar_w4(g1_b, p->rw); });
            p->g_c = zl::mul_scalar_w4(g_a, p->sw);
            t_rb.join();
            zl::add_full(p->g_c, rb);
        }
        zl::add_full(p->g_c, p->rs_delta);
        store_canon<G1>(p->a_words, &p->a_inf, g_a);  // A is final: its normalisation (one inversion) leaves the critical path too
        p->have_c = true;
        p->lap("s A + r B1 done");
    };
    return ZL_DISPATCH(p->pk->curve, ZL_G1, zl_msm_run_jobs, p->ctx, jb, jf, js, jn, jw, 4, &p->g1_sums[0][0], (const std::atomic<int>*)&p->h_recorded, &on_done);
}
// Host assembly: A (and, in the four-MSM form, s A + r B1 - r s delta1) were formed by the completion callback and B by the G2 worker; C needs the last MSMs --
// every sum of it in the folded form's second job, l and h in the four-MSM form's third and fourth
template <class G1, class G2>
static void g16_assemble(G16Proof<G1, G2>* p, zl_g16_proof* out) {
    using F1 = typename G1::F;
    zl::add_full(p->g_c, from_partial<F1>(p->g1_sums[p->fold ? 1 : 2]));
    if (!p->fold) zl::add_full(p->g_c, from_partial<F1>(p->g1_sums[3]));
    p->lap("assembly");
    memset(out, 0, sizeof *out);
    memcpy(out->a, p->a_words, sizeof p->a_words);
    out->a_inf = p->a_inf;
    memcpy(out->b, p->b_words, sizeof p->b_words);
    out->b_inf = p->b_inf;
    store_canon<G1>(out->c, &out->c_inf, p->g_c);
    p->lap("proof normalised");
}

template <class G1, class G2>
static int groth16_prove_t(zl_ctx* ctx, const zl_g16_pk* pk, const zl_r1cs_dev* cs, const uint64_t* assignment, unsigned flags, const uint64_t* r,
                           const uint64_t* s, zl_g16_proof* out, const uint64_t* witness = nullptr) {
    G16Shape sh;
    int rc;
    if ((rc = g16_shape<typename G1::FrP>(cs, &sh))) return rc;
    G16Proof<G1, G2> p(ctx, pk, cs, sh);
    if ((rc = g16_key_handles(ctx, pk, sh, p.bs))) return rc;
    // a small proof's C comes from ONE folded query (G16KeyCache above)
    const bool fold = sh.log_n <= (unsigned)zl_tune("ZL_TUNE_G16_FOLD_LOG_N", ZL_G16_FOLD_LOG_N);
    if ((rc = g16_stage(&p, assignment, witness, flags, r, s, fold, 1))) return rc;
    g16_issue_witness_map(&p);
    // (every return below first waits for that thread: it works on this frame)
    auto wm_fail = [&](int code) { (void)p.join_witness_map(); ctx->timing_on = p.timing_saved; return code; };
    if ((rc = g16_first_points(&p))) return wm_fail(rc);
    // the key's host tables (and, for a small proof, its folded C query): built by the first proof over the key
    if ((rc = g16_key_cache<G1, G2>(ctx, pk, p.bs, fold, sh.nv, sh.nw, (size_t)sh.N - 1, &p.kc))) return wm_fail(rc);
    g16_start_fixed_base(&p);
    p.lap("z on device, host pre started");
    g16_issue_g2(&p);
    rc = fold ? g16_run_g1_folded(&p) : g16_run_g1_four(&p);
    p.lap("G1 pipeline returned");
    (void)p.join_witness_map();  // also on the error path: nothing of this proof may still be running
    zl_ctx_worker(ctx, 1).wait();
    if (!rc) rc = p.rc_wm;
    p.lap("G2 joined");
    if (p.pre.joinable()) p.pre.join();
    if (p.pre_g2.joinable()) p.pre_g2.join();
    if (!rc) rc = p.rc_g2;
    if (!rc && !p.have_c) rc = ZL_EHIP;  // (the completion callback did not run: cannot happen after a successful pipeline)
    ctx->timing_on = p.timing_saved;
    if (rc) return rc;
    if (ctx->timing_on) {
        ZL_HIP(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
        ZL_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->timing = zl_timing{};
        ZL_HIP(ctx, hipEventElapsedTime(&ctx->timing.total_ms, ctx->ev[0], ctx->ev[1]));
        ctx->timing.launches = 5;
    }
    ctx->g16_h = p.d_h;
    ctx->g16_h_n = sh.N;
    g16_assemble(&p, out);
    return ZL_OK;
}

// ---- one proof over the G devices of an mctx ---------------------------------------------------------------------------
// Rank g holds, on zl_mctx_ctx(m, g), bases handles with ITS contiguous slice of every query (zl_g16_shard); rank 0 also holds the constraint matrices.
//   1. rank 0: assignment -> device, witness map (spmv, 7 NTTs) -> h                                        (g16_stage, g16_issue_witness_map; the key's handles are not looked at)
//   2. every rank, on its own host thread: its slices of z and h arrive by device-to-device copy, then its five partial MSMs (a, b1, l, h in G1 and b2
//      in G2) through the single-device pipeline (zl_msm_run) -> five un-normalised partial sums per rank
//   3. host: the partials of each MSM are folded over the ranks (what an all-gather + fold does between processes: EC addition is not a collective's
//      reduce op) and the proof is assembled exactly as the single-device prover does
// Same proof, byte for byte, as zl_groth16_prove_resident with the same (r, s) (tests/test_gpu_multi.py).  Functional: the MSM phase of a proof shards like
// any MSM (512 B of partials per rank and MSM); the witness map stays on one device (the NTTs of one proof are replicas work, not sharded work).
template <class G1, class G2>
static int groth16_prove_sharded_t(zl_mctx* m, const zl_g16_pk* pk, const zl_g16_shard* shards, const zl_r1cs_dev* cs, const uint64_t* assignment, unsigned flags,
                                   const uint64_t* r, const uint64_t* s, zl_g16_proof* out) {
    using FrP = typename G1::FrP;
    using F1 = typename G1::F;
    using F2 = typename G2::F;
    const int G = zl_mctx_size(m);
    zl_ctx* ctx0 = zl_mctx_ctx(m, 0);
    G16Shape sh;
    int rc;
    if ((rc = g16_shape<FrP>(cs, &sh))) return rc;
    const uint32_t ni = sh.ni, nw = sh.nw, nv = sh.nv;
    const size_t N = sh.N;
    // the slices must tile [0, nv), [0, nw) and [0, N - 1) in rank order
    size_t v = 0, w = 0, hq = 0;
    for (int g = 0; g < G; g++) {
        if (shards[g].var_first != v || shards[g].wit_first != w || shards[g].h_first != hq) return ZL_EINVAL;
        v += shards[g].var_count; w += shards[g].wit_count; hq += shards[g].h_count;
    }
    if (v != nv || w != nw || hq != N - 1) return ZL_EINVAL;
    ZL_HIP(ctx0, hipSetDevice(ctx0->device));
    {   // step 1: no MSM follows on this ctx, so no folded scalars, the transforms' faster passes, and the host waits for h
        G16Proof<G1, G2> p(ctx0, pk, cs, sh);
        if ((rc = g16_stage(&p, assignment, nullptr, flags, r, s, false, 0))) return rc;
        g16_issue_witness_map(&p);
        const hipError_t e1 = p.join_witness_map(), e2 = hipStreamSynchronize(ctx0->stream);
        ctx0->timing_on = p.timing_saved;
        if (p.rc_wm) return p.rc_wm;
        if (e1 != hipSuccess || e2 != hipSuccess) { ctx0->last_hip = (int)(e1 != hipSuccess ? e1 : e2); return ZL_EHIP; }
        ctx0->g16_h = p.d_h;
        ctx0->g16_h_n = N;
        ctx0->g16_z = p.d_zc;
    }
    const unsigned char* d_z0 = reinterpret_cast<const unsigned char*>(ctx0->g16_z);
    const unsigned char* d_h0 = reinterpret_cast<const unsigned char*>(ctx0->g16_h);
    std::vector<std::array<uint64_t, 5 * ZL_PARTIAL_WORDS>> parts((size_t)G);
    std::vector<int> rcs((size_t)G, ZL_OK);
    std::vector<std::thread> th;
    for (int g = 0; g < G; g++)
        th.emplace_back([&, g]() {
            zl_ctx* c = zl_mctx_ctx(m, g);
            const zl_g16_shard& sh = shards[g];
            auto fail = [&](int code) { rcs[(size_t)g] = code; };
            if (hipSetDevice(c->device) != hipSuccess) return fail(ZL_EHIP);
            // this rank's scalars: [variables | witnesses | quotient coefficients], canonical, copied from rank 0's device
            void* d = nullptr;
            const size_t nvar = sh.var_count, nwit = sh.wit_count, nh = sh.h_count;
            int r2 = zl_scratch_get(c, ZL_SLOT_STAGING, (nvar + nwit + nh + 1) * 32, &d);
            if (r2) return fail(r2);
            unsigned char* ds = reinterpret_cast<unsigned char*>(d);
            hipError_t e = hipSuccess;
            if (nvar) e = hipMemcpyPeerAsync(ds, c->device, d_z0 + sh.var_first * 32, ctx0->device, nvar * 32, c->stream);
            if (e == hipSuccess && nwit) e = hipMemcpyPeerAsync(ds + nvar * 32, c->device, d_z0 + ((size_t)ni + sh.wit_first) * 32, ctx0->device, nwit * 32, c->stream);
            if (e == hipSuccess && nh) e = hipMemcpyPeerAsync(ds + (nvar + nwit) * 32, c->device, d_h0 + sh.h_first * 32, ctx0->device, nh * 32, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) { c->last_hip = (int)e; return fail(ZL_EHIP); }
            const struct { uint64_t handle; int group; const unsigned char* sc; size_t n; } jobs[5] = {
                {sh.a_query, ZL_G1, ds, nvar}, {sh.b_g1_query, ZL_G1, ds, nvar}, {sh.h_query, ZL_G1, ds + (nvar + nwit) * 32, nh},
                {sh.l_query, ZL_G1, ds + nvar * 32, nwit}, {sh.b_g2_query, ZL_G2, ds, nvar}};
            for (int j = 0; j < 5; j++) {
                uint64_t* outp = parts[(size_t)g].data() + (size_t)j * ZL_PARTIAL_WORDS;
                memset(outp, 0, ZL_PARTIAL_WORDS * 8);
                if (jobs[j].n == 0) {  // an empty slice contributes the point at infinity
                    if (jobs[j].group == ZL_G1) { const XYZZ<F1> z = XYZZ<F1>::inf(); memcpy(outp, &z, sizeof z); }
                    else { const XYZZ<F2> z = XYZZ<F2>::inf(); memcpy(outp, &z, sizeof z); }
                    continue;
                }
                auto it = c->bases.find(jobs[j].handle);
                if (it == c->bases.end() || it->second.curve != (int)pk->curve || it->second.group != jobs[j].group || it->second.n < jobs[j].n) return fail(ZL_EHANDLE);
                r2 = ZL_DISPATCH(pk->curve, jobs[j].group, zl_msm_run, c, it->second, 0, jobs[j].sc, jobs[j].n, outp);
                if (r2) return fail(r2);
            }
        });
    for (auto& t : th) t.join();
    for (int g = 0; g < G; g++)
        if (rcs[(size_t)g]) return rcs[(size_t)g];
    // fold over the ranks, then the assembly of create_proof_with_assignment
    XYZZ<F1> sum1[4];
    XYZZ<F2> sum2 = XYZZ<F2>::inf();
    for (auto& x : sum1) x = XYZZ<F1>::inf();
    for (int g = 0; g < G; g++) {
        for (int j = 0; j < 4; j++) zl::add_full(sum1[j], from_partial<F1>(parts[(size_t)g].data() + (size_t)j * ZL_PARTIAL_WORDS));
        zl::add_full(sum2, from_partial<F2>(parts[(size_t)g].data() + (size_t)4 * ZL_PARTIAL_WORDS));
    }
    uint32_t rw[8], sw[8], rsw[8];
    memcpy(rw, r, 32);
    memcpy(sw, s, 32);
    g16_rs<FrP>(rw, sw, rsw);
    const XYZZ<F1> delta1 = affine_from_canon<G1>(pk->delta_g1);
    const XYZZ<F2> delta2 = affine_from_canon<G2>(pk->delta_g2);
    // (the ranks' MSMs start at index 0 of their slices: no first point to add)
    const XYZZ<F1> g_a = g16_blinded_sum<G1>(zl::mul_scalar_w4(delta1, rw), nullptr, sum1[0], pk->alpha_g1);   // A = alpha + sum z_i a_i + r delta
    const XYZZ<F1> g1_b = g16_blinded_sum<G1>(zl::mul_scalar_w4(delta1, sw), nullptr, sum1[1], pk->beta_g1);   // B1 = beta + sum z_i b_i + s delta
    const XYZZ<F2> g2_b = g16_blinded_sum<G2>(zl::mul_scalar_w4(delta2, sw), nullptr, sum2, pk->beta_g2);      // B = the same in G2
    XYZZ<F1> g_c = zl::mul_scalar_w4(g_a, sw);              // C = s A + r B1 - r s delta + sum_w z_w l_w + sum h_i H_i
    zl::add_full(g_c, zl::mul_scalar_w4(g1_b, rw));
    XYZZ<F1> rs_delta = zl::mul_scalar_w4(delta1, rsw);
    zl::neg_inplace(rs_delta);
    zl::add_full(g_c, rs_delta);
    zl::add_full(g_c, sum1[3]);
    zl::add_full(g_c, sum1[2]);
    memset(out, 0, sizeof *out);
    store_canon<G1>(out->a, &out->a_inf, g_a);
    store_canon<G2>(out->b, &out->b_inf, g2_b);
    store_canon<G1>(out->c, &out->c_inf, g_c);
    return ZL_OK;
}
extern "C" int zl_groth16_prove_sharded(zl_mctx* m, const zl_g16_pk* pk, const zl_g16_shard* shards, uint64_t r1cs_handle_rank0, const uint64_t* assignment,
                                        unsigned flags, const uint64_t* r, const uint64_t* s, zl_g16_proof* out) {
    if (!m || !pk || !shards || !assignment || !r || !s || !out || (flags & ~ZL_MONT)) return ZL_EINVAL;
    zl_ctx* ctx0 = zl_mctx_ctx(m, 0);
    if (!ctx0) return ZL_EINVAL;
    const zl_r1cs_dev* rd = nullptr;
    const int rc = g16_entry(ctx0, pk, r1cs_handle_rank0, r, s, 1, &rd);
    if (rc) return rc;
    if (pk->curve == ZL_BLS12_381) return groth16_prove_sharded_t<BlsG1, BlsG2>(m, pk, shards, rd, assignment, flags, r, s, out);
    if (pk->curve == ZL_BN254) return groth16_prove_sharded_t<BnG1, BnG2>(m, pk, shards, rd, assignment, flags, r, s, out);
    return ZL_EINVAL;
}

// Full structural validation of a caller-supplied CSR, once per upload (O(nnz) on the host): row_ptr starts at 0 and is monotone,
// every column index names a variable.  k_r1cs_spmv then never reads val / z out of bounds, whatever the caller passed.
static bool r1cs_view_ok(const zl_r1cs* cs) {
    if (!cs || cs->n_instance < 1) return false;
    const uint64_t nv = (uint64_t)cs->n_instance + cs->n_witness;
    if (nv >= (1ull << 31)) return false;
    for (int m = 0; m < 3; m++) {
        const uint32_t* rp = cs->row_ptr[m];
        if (!rp || rp[0] != 0) return false;
        for (uint32_t i = 0; i < cs->n_constraints; i++)
            if (rp[i + 1] < rp[i]) return false;
        const uint32_t nnz = rp[cs->n_constraints];
        if (nnz && (!cs->col[m] || !cs->val[m])) return false;
        for (uint32_t k = 0; k < nnz; k++)
            if (cs->col[m][k] >= nv) return false;
    }
    return true;
}
extern "C" int zl_r1cs_upload(zl_ctx* ctx, zl_curve_t curve, const zl_r1cs* cs, uint64_t* handle_out) {
    if (!ctx || !handle_out || !r1cs_view_ok(cs)) return ZL_EINVAL;
    if (curve != ZL_BLS12_381 && curve != ZL_BN254) return ZL_EINVAL;
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    zl_r1cs_dev dev{};
    dev.curve = curve;
    const int rc = curve == ZL_BLS12_381 ? r1cs_upload_t<BLS12_381_Fr>(ctx, cs, &dev) : r1cs_upload_t<BN254_Fr>(ctx, cs, &dev);
    if (rc) return rc;
    uint64_t h;
    {
        std::unique_lock<std::shared_mutex> lk(ctx->maps_mu);
        h = ctx->next_handle++;
        ctx->r1cs[h] = dev;
    }
    *handle_out = h;
    return ZL_OK;
}
extern "C" int zl_r1cs_free(zl_ctx* ctx, uint64_t handle) {
    if (!ctx) return ZL_EINVAL;
    auto it = ctx->r1cs.find(handle);
    if (it == ctx->r1cs.end()) return ZL_EHANDLE;
    zl_ctx_release_idle_lane(ctx);
    if (ctx->forks.load() > 0) return ZL_EINVAL;  // a fork may be reading it: destroy the forks first
    ZL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (it->second.d_base) (void)hipFree(it->second.d_base);
    ctx->r1cs.erase(it);
    return ZL_OK;
}
extern "C" int zl_groth16_prove_resident(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, const uint64_t* assignment, unsigned flags,
                                         const uint64_t* r, const uint64_t* s, zl_g16_proof* out) {
    if (!ctx || !pk || !assignment || !r || !s || !out || (flags & ~ZL_MONT)) return ZL_EINVAL;
    const zl_r1cs_dev* rd = nullptr;
    const int rc = g16_entry(ctx, pk, r1cs_handle, r, s, 1, &rd);
    if (rc) return rc;
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    if (pk->curve == ZL_BLS12_381) return groth16_prove_t<BlsG1, BlsG2>(ctx, pk, rd, assignment, flags, r, s, out);
    if (pk->curve == ZL_BN254) return groth16_prove_t<BnG1, BnG2>(ctx, pk, rd, assignment, flags, r, s, out);
    return ZL_EINVAL;
}
// internal (zl_host.hip): the assignment as the compiler holds it -- instance block and witness block, Montgomery limbs
int zl_groth16_prove_split(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, const uint64_t* instance, const uint64_t* witness, const uint64_t* r,
                           const uint64_t* s, zl_g16_proof* out) {
    if (!ctx || !pk || !instance || !r || !s || !out) return ZL_EINVAL;
    const zl_r1cs_dev* rd = nullptr;
    const int rc = g16_entry(ctx, pk, r1cs_handle, r, s, 1, &rd);
    if (rc) return rc;
    if (rd->n_witness && !witness) return ZL_EINVAL;
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    static const uint64_t none[4] = {0, 0, 0, 0};
    if (pk->curve == ZL_BLS12_381) return groth16_prove_t<BlsG1, BlsG2>(ctx, pk, rd, instance, ZL_MONT, r, s, out, witness ? witness : none);
    if (pk->curve == ZL_BN254) return groth16_prove_t<BnG1, BnG2>(ctx, pk, rd, instance, ZL_MONT, r, s, out, witness ? witness : none);
    return ZL_EINVAL;
}
extern "C" int zl_groth16_prove(zl_ctx* ctx, const zl_g16_pk* pk, const zl_r1cs* cs, const uint64_t* assignment, const uint64_t* r, const uint64_t* s,
                                zl_g16_proof* out) {
    if (!ctx || !pk || !r || !s || !r1cs_view_ok(cs)) return ZL_EINVAL;
    int rc = g16_blinding_ok(pk->curve, r, s, 1);  // (also in zl_groth16_prove_resident: here before the matrices go up)
    if (rc) return rc;
    uint64_t h = 0;
    rc = zl_r1cs_upload(ctx, pk->curve, cs, &h);
    if (rc) return rc;
    rc = zl_groth16_prove_resident(ctx, pk, h, assignment, ZL_CANON, r, s, out);
    (void)zl_r1cs_free(ctx, h);
    return rc;
}

// ---- many proofs over one key in one device pass (zl_groth16_prove_batch) -------------------------------------------------------------------------------------
// The single small proof is ~16 launches of kernels that occupy a handful of workgroups, three MSMs of a few hundred points and six fixed-base products on host
// threads.  A batch of witnesses over one key turns every one of those into ONE launch with a batch dimension:
//   * witness map (g16_witness_map, count = chunk): a, b, c laid out [3][chunk][N]; the two transform steps are one zl_ntt_run_batch of 3 chunk vectors each, the pointwise step runs over chunk N
//     elements, the coset inverse is one more batch call;
//   * the whole proof inside three multi-MSMs (zl_msm_multi.hip) over extended queries cached with the key:
//       A = <(1, z_1.., r, 1),                      a | delta1 | alpha1>
//       B = <(1, z_1.., s, 1),                      b2 | delta2 | beta2>
//       C = <(z_w | s z | r z | h | s | r | r s),   l | a | b1 | h | alpha1 | beta1 | delta1>      (the folded form of C above with its three fixed-base terms inside)
//     so the host does no point arithmetic and the proofs come back canonical.  Variable 0 enters unscaled as in k_g16_fold_scalars.
// The three scalar matrices of a chunk, proof v = blockIdx.y (zc canonical, zm Montgomery, h Montgomery as the coset inverse leaves it; r, s canonical):
//   sa[v] = (1, z_1.., r, 1)   sb[v] = (1, z_1.., s, 1)   sc[v] = (z_w | s z | r z | h[0 .. N - 1) | s | r | r s)
template <class FrP>
__global__ void __launch_bounds__(256) k_g16_batch_scalars(const Fp<FrP>* __restrict__ zc_all, const Fp<FrP>* __restrict__ zm_all, const Fp<FrP>* __restrict__ h_all,
                                                            const Fp<FrP>* __restrict__ r_all, const Fp<FrP>* __restrict__ s_all, uint32_t ni, uint32_t nv, uint32_t N,
                                                            Fp<FrP>* __restrict__ sa_all, Fp<FrP>* __restrict__ sb_all, Fp<FrP>* __restrict__ sc_all) {
    using F = Fp<FrP>;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, v = blockIdx.y;
    const uint32_t nw = nv - ni, na = nv + 2, nc = nw + 2 * nv + (N - 1) + 3;
    const F r = r_all[v], s = s_all[v];
    F* sa = sa_all + (size_t)v * na;
    F* sb = sb_all + (size_t)v * na;
    F* sc = sc_all + (size_t)v * nc;
    const F one = zl::from_mont(F::one());
    if (i < nv) {
        const F c = zc_all[(size_t)v * nv + i], m = zm_all[(size_t)v * nv + i];
        sa[i] = i ? c : one;
        sb[i] = i ? c : one;
        sc[nw + i] = i ? zl::mul(m, s) : s;        // (z R) s / R = z s, canonical
        sc[nw + nv + i] = i ? zl::mul(m, r) : r;
        if (i >= ni) sc[i - ni] = c;
    }
    if (i < N - 1) sc[nw + 2 * nv + i] = zl::from_mont(h_all[(size_t)v * N + i]);
    if (i == 0) {
        sa[nv] = r; sa[nv + 1] = one;
        sb[nv] = s; sb[nv + 1] = one;
        F* t = sc + nw + 2 * nv + (N - 1);
        t[0] = s; t[1] = r;
        t[2] = zl::mul(zl::to_mont(r), s);         // (r R) s / R = r s, canonical
    }
}

// The three extended queries of a key, cached in its G16KeyCache.  They are built OUTSIDE zl_bases_cache_mutex (uploads, device copies and two synchronisations:
// a lane that proves over another key must not wait for them) and installed under it; when two lanes build them for one key at once, the second one's are dropped.
template <class G1, class G2>
static int g16_batch_queries(zl_ctx* ctx, const zl_g16_pk* pk, const zl_bases* const* bs, size_t nv, size_t nw, size_t nh, std::shared_ptr<G16KeyCache<G1, G2>>* out) {
    using KC = G16KeyCache<G1, G2>;
    std::shared_ptr<KC> kc;
    int rc = g16_key_cache<G1, G2>(ctx, pk, bs, false, nv, nw, nh, &kc);
    if (rc) return rc;
    const uint64_t hs[5] = {pk->a_query, pk->b_g1_query, pk->h_query, pk->l_query, pk->b_g2_query};
    auto fits = [&](const KC& k) { return k.bq_built && k.bq_nv == nv && k.bq_nw == nw && k.bq_nh == nh && !memcmp(k.bq_handles, hs, sizeof hs); };
    {
        std::lock_guard<std::mutex> lk(zl_bases_cache_mutex());
        if (fits(*kc)) { *out = kc; return ZL_OK; }
    }
    constexpr size_t W1 = 2 * FieldIO<typename G1::F>::WORDS, W2 = 2 * FieldIO<typename G2::F>::WORDS;
    std::vector<uint32_t> fx1(3 * W1), fx2(2 * W2);  // delta1 | alpha1 | beta1 and delta2 | beta2, canonical
    memcpy(&fx1[0], pk->delta_g1, W1 * 4);
    memcpy(&fx1[W1], pk->alpha_g1, W1 * 4);
    memcpy(&fx1[2 * W1], pk->beta_g1, W1 * 4);
    memcpy(&fx2[0], pk->delta_g2, W2 * 4);
    memcpy(&fx2[W2], pk->beta_g2, W2 * 4);
    zl_bases t1, t2, q[3];
    rc = ZL_DISPATCH(pk->curve, ZL_G1, zl_bases_upload, ctx, fx1.data(), 3, 0, -1, 0, &t1);
    if (!rc) rc = ZL_DISPATCH(pk->curve, ZL_G2, zl_bases_upload, ctx, fx2.data(), 2, 0, -1, 0, &t2);
    if (!rc) {
        const zl_bases* parts[3] = {bs[0], &t1, &t1};
        const size_t first[3] = {0, 0, 1}, n[3] = {nv, 1, 1};
        rc = ZL_DISPATCH(pk->curve, ZL_G1, zl_bases_concat, ctx, parts, first, n, 3, &q[0]);
    }
    if (!rc) {
        const zl_bases* parts[3] = {bs[4], &t2, &t2};
        const size_t first[3] = {0, 0, 1}, n[3] = {nv, 1, 1};
        rc = ZL_DISPATCH(pk->curve, ZL_G2, zl_bases_concat, ctx, parts, first, n, 3, &q[1]);
    }
    if (!rc) {
        const zl_bases* parts[7] = {bs[3], bs[0], bs[1], bs[2], &t1, &t1, &t1};
        const size_t first[7] = {0, 0, 0, 0, 1, 2, 0}, n[7] = {nw, nv, nv, nh, 1, 1, 1};
        rc = ZL_DISPATCH(pk->curve, ZL_G1, zl_bases_concat, ctx, parts, first, n, 7, &q[2]);
    }
    KC::free_bases(t1);
    KC::free_bases(t2);
    if (rc) {
        for (zl_bases& b : q) KC::free_bases(b);
        return rc;
    }
    for (int i = 0; i < 3; i++) { q[i].curve = (int)pk->curve; q[i].group = i == 1 ? ZL_G2 : ZL_G1; }
    std::lock_guard<std::mutex> lk(zl_bases_cache_mutex());
    {   // (a folded proof on another lane may have put a fresh cache object in place meanwhile)
        std::shared_ptr<KC> now = std::static_pointer_cast<KC>(bs[3]->g16_cache);
        if (now && now->key_words == kc->key_words) kc = now;
    }
    if (fits(*kc)) {
        for (zl_bases& b : q) KC::free_bases(b);
    } else if (kc->bq_built && kc.use_count() > 2) {
        // another lane still proves with the queries of another shape: keep them with their object, hang ours on a fresh one
        kc = kc->fresh_with_tables();
        bs[3]->g16_cache = kc;
    }
    if (!fits(*kc)) {
        kc->drop_batch();
        for (int i = 0; i < 3; i++) kc->bq[i] = q[i];
        memcpy(kc->bq_handles, hs, sizeof hs);
        kc->bq_nv = nv;
        kc->bq_nw = nw;
        kc->bq_nh = nh;
        kc->bq_built = true;
    }
    *out = kc;
    return ZL_OK;
}

// Dispatch bounds, from the interleaved measurement against the zl_groth16_prove_circuits stream (profiles/prove_batch_bench.log; worst pairing of repetitions):
// domain 2^8 (235 constraints) 1.70x / 6.99x / 8.57x at 64 / 1 024 / 16 384 proofs on BLS12-381, 2.32x / 9.57x / 11.8x on BN254; domain 2^11 (1 873) 1.37x / 2.94x
// and 1.14x / 4.00x at 64 / 1 024; domain 2^14 (14 977) 0.75 - 0.82x: a loss.  Nothing was measured between 2^11 and 2^14 or below 64 proofs, so the bounds stop there.
#define ZL_G16_BATCH_LOG_N 11  // largest domain (log2) whose batches stay on the device (ZL_TUNE_G16_BATCH_LOG_N)
#define ZL_G16_BATCH_MIN 64    // ... from this many proofs on (ZL_TUNE_G16_BATCH_MIN)
#define ZL_G16_BATCH_BUDGET ((size_t)512 << 20)  // bytes of ZL_SLOT_G16_BATCH a chunk may take

// Where the assignments of a batch come from: host memory (zl_groth16_prove_batch: one upload per chunk), device memory (zl_groth16_prove_batch_dev: one
// device-to-device copy per chunk), or a producer (zl_groth16_prove_poseidon_chains, zl_groth16_prove_merkle_paths / _members) that writes the `ch` canonical rows of the chunk from proof c0 on in place
// (fill_dev: into the chunk's block of ZL_SLOT_G16_BATCH, on ctx->stream, finished on return) -- and, for the loop over the resident prover, into host rows.
struct G16BatchSource {
    const uint64_t* host = nullptr;
    const uint64_t* dev = nullptr;
    std::function<int(size_t c0, size_t ch, void* d_rows)> fill_dev;
    std::function<int(size_t c0, size_t ch, uint64_t* rows)> fill_host;
};
#define ZL_G16_BATCH_HOST_STAGE ((size_t)64 << 20)  // bytes of host staging the resident loop takes for assignments that are not in host memory

template <class G1, class G2>
static int groth16_prove_batch_dev_t(zl_ctx* ctx, const zl_g16_pk* pk, const zl_r1cs_dev* cs, const zl_bases* const* bs, const G16Shape& sh, const G16BatchSource& src,
                                     unsigned flags, const uint64_t* r, const uint64_t* s, size_t count, zl_g16_proof* proofs) {
    using FrP = typename G1::FrP;
    using Fr = Fp<FrP>;
    const uint32_t ni = sh.ni, nw = sh.nw, nv = sh.nv, N = sh.N;
    std::shared_ptr<G16KeyCache<G1, G2>> kc;
    int rc = g16_batch_queries<G1, G2>(ctx, pk, bs, nv, nw, (size_t)N - 1, &kc);
    if (rc) return rc;
    const size_t na = (size_t)nv + 2, ncs = (size_t)nw + 2 * (size_t)nv + (N - 1) + 3;
    // per proof: z canonical + Montgomery, a | b | c, r, s, the three scalar rows
    const size_t per = ((size_t)2 * nv + (size_t)3 * N + 2 + 2 * na + ncs) * 32;
    size_t chunk = std::max<size_t>(1, ZL_G16_BATCH_BUDGET / per);
    const int forced = zl_tune("ZL_TUNE_G16_BATCH_CHUNK", 0);
    if (forced > 0) chunk = (size_t)forced;
    chunk = std::min(std::min(chunk, count), std::min<size_t>(65535 / 3, (size_t)0x7fffffffu / std::max<size_t>(N, ncs)));  // three vectors per proof in one transform call; 32-bit element counts
    if (chunk < 1) return ZL_EINVAL;
    void* base;
    if ((rc = zl_scratch_get(ctx, ZL_SLOT_G16_BATCH, chunk * per + 256, &base))) return rc;
    Fr* d_zc = reinterpret_cast<Fr*>(base);
    Fr* d_zm = d_zc + chunk * nv;
    Fr* d_abc = d_zm + chunk * nv;  // [3][ch][N] for the ch proofs of the chunk in flight
    Fr* d_r = d_abc + chunk * 3 * N;
    Fr* d_s = d_r + chunk;
    Fr* d_sa = d_s + chunk;
    Fr* d_sb = d_sa + chunk * na;
    Fr* d_sc = d_sb + chunk * na;
    hipStream_t st = ctx->stream;
    ctx->g16_h = nullptr;  // no single quotient to hand out after a batch
    ctx->g16_h_n = 0;
    const int timing_saved = ctx->timing_on;
    ctx->timing_on = 0;  // the inner calls must not record into the ctx's events
    constexpr size_t W1 = FieldIO<typename G1::F>::WORDS, W2 = FieldIO<typename G2::F>::WORDS;  // u64 words of a canonical G1 / G2 point (2 coordinates of WORDS u32)
    std::vector<uint64_t> xa(chunk * W1), xb(chunk * W2), xc(chunk * W1);
    std::vector<uint8_t> ia(chunk), ib(chunk), ic(chunk);
    auto body = [&]() -> int {
        for (size_t c0 = 0; c0 < count; c0 += chunk) {
            const uint32_t ch = (uint32_t)std::min(chunk, count - c0);
            const uint32_t tot_z = ch * nv;
            Fr* d_in = (flags & ZL_MONT) ? d_zm : d_zc;
            if (src.fill_dev) {
                const int e = src.fill_dev(c0, ch, d_in);
                if (e) return e;
            } else {
                const uint64_t* from = (src.dev ? src.dev : src.host) + c0 * (size_t)nv * 4;
                ZL_HIP(ctx, hipMemcpyAsync(d_in, from, (size_t)tot_z * 32, src.dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
            }
            ZL_HIP(ctx, hipMemcpyAsync(d_r, r + c0 * 4, (size_t)ch * 32, hipMemcpyHostToDevice, st));
            ZL_HIP(ctx, hipMemcpyAsync(d_s, s + c0 * 4, (size_t)ch * 32, hipMemcpyHostToDevice, st));
            int e;
            if ((e = g16_z_forms<FrP>(ctx, d_zc, d_zm, tot_z, flags))) return e;
            if ((e = g16_witness_map<FrP>(ctx, pk->curve, cs, d_zm, nv, ch, d_abc, sh.log_n))) return e;
            hipLaunchKernelGGL((k_g16_batch_scalars<FrP>), dim3((std::max(nv, N) + 255) / 256, ch), dim3(256), 0, st, d_zc, d_zm, d_abc, d_r, d_s, ni, nv, N, d_sa, d_sb, d_sc);
            ZL_HIP(ctx, hipGetLastError());
            if ((e = ZL_DISPATCH(pk->curve, ZL_G1, zl_msm_multi_run, ctx, kc->bq[0], 0, d_sa, na, na, ch, xa.data(), ia.data()))) return e;
            if ((e = ZL_DISPATCH(pk->curve, ZL_G2, zl_msm_multi_run, ctx, kc->bq[1], 0, d_sb, na, na, ch, xb.data(), ib.data()))) return e;
            if ((e = ZL_DISPATCH(pk->curve, ZL_G1, zl_msm_multi_run, ctx, kc->bq[2], 0, d_sc, ncs, ncs, ch, xc.data(), ic.data()))) return e;
            for (uint32_t j = 0; j < ch; j++) {
                zl_g16_proof* p = proofs + c0 + j;
                memset(p, 0, sizeof *p);
                memcpy(p->a, &xa[j * W1], W1 * 8);
                memcpy(p->b, &xb[j * W2], W2 * 8);
                memcpy(p->c, &xc[j * W1], W1 * 8);
                p->a_inf = ia[j];
                p->b_inf = ib[j];
                p->c_inf = ic[j];
            }
        }
        return ZL_OK;
    };
    rc = body();
    if (rc) (void)hipStreamSynchronize(st);  // nothing of the batch may still be running when the caller sees the error
    ctx->timing_on = timing_saved;
    return rc;
}

template <class G1, class G2>
static int groth16_prove_batch_t(zl_ctx* ctx, const zl_g16_pk* pk, const zl_r1cs_dev* cs, const G16BatchSource& src, unsigned flags, const uint64_t* r,
                                 const uint64_t* s, size_t count, zl_g16_proof* proofs) {
    // the resident prover's checks, so that both paths answer a bad circuit or key alike
    G16Shape sh;
    const zl_bases* bs[5];
    int rc0;
    if ((rc0 = g16_shape<typename G1::FrP>(cs, &sh)) || (rc0 = g16_key_handles(ctx, pk, sh, bs))) return rc0;
    const size_t nv = sh.nv;
    if (sh.log_n <= (unsigned)zl_tune("ZL_TUNE_G16_BATCH_LOG_N", ZL_G16_BATCH_LOG_N) && count >= (size_t)std::max(1, zl_tune("ZL_TUNE_G16_BATCH_MIN", ZL_G16_BATCH_MIN)))
        return groth16_prove_batch_dev_t<G1, G2>(ctx, pk, cs, bs, sh, src, flags, r, s, count, proofs);
    // The resident prover takes its assignment from host memory: assignments that live on the device, or that a producer makes, come through host staging
    // of at most ZL_G16_BATCH_HOST_STAGE bytes at a time.
    const size_t block = src.host ? count : std::min(count, std::max<size_t>(1, ZL_G16_BATCH_HOST_STAGE / (nv * 32)));
    std::vector<uint64_t> staged(src.host ? 0 : block * nv * 4);
    for (size_t c0 = 0; c0 < count; c0 += block) {
        const size_t ch = std::min(block, count - c0);
        const uint64_t* rows = src.host;
        if (!src.host) {
            if (src.dev) {
                ZL_HIP(ctx, hipMemcpyAsync(staged.data(), src.dev + c0 * nv * 4, ch * nv * 32, hipMemcpyDeviceToHost, ctx->stream));
                ZL_HIP(ctx, hipStreamSynchronize(ctx->stream));
            } else {
                const int rc = src.fill_host(c0, ch, staged.data());
                if (rc) return rc;
            }
            rows = staged.data();
        }
        for (size_t j = c0; j < c0 + ch; j++) {
            const int rc = groth16_prove_t<G1, G2>(ctx, pk, cs, rows + (src.host ? j : j - c0) * nv * 4, flags, r + 4 * j, s + 4 * j, proofs + j);
            if (rc) return rc;
        }
    }
    return ZL_OK;
}
static int groth16_prove_batch_any(zl_ctx* ctx, const zl_g16_pk* pk, const zl_r1cs_dev* rd, const G16BatchSource& src, unsigned flags, const uint64_t* r, const uint64_t* s,
                                   size_t count, zl_g16_proof* proofs) {
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    if (pk->curve == ZL_BLS12_381) return groth16_prove_batch_t<BlsG1, BlsG2>(ctx, pk, rd, src, flags, r, s, count, proofs);
    if (pk->curve == ZL_BN254) return groth16_prove_batch_t<BnG1, BnG2>(ctx, pk, rd, src, flags, r, s, count, proofs);
    return ZL_EINVAL;
}
// the assignments of the batch are rows in host or device memory
static int groth16_prove_batch_rows(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, const void* rows, bool on_device, unsigned flags, const uint64_t* r,
                                    const uint64_t* s, size_t count, zl_g16_proof* proofs) {
    if (!ctx || !pk || (flags & ~ZL_MONT) || (count && (!rows || !r || !s || !proofs))) return ZL_EINVAL;
    const zl_r1cs_dev* rd = nullptr;
    const int rc = g16_entry(ctx, pk, r1cs_handle, r, s, count, &rd);
    if (rc || count == 0) return rc;
    G16BatchSource src;
    (on_device ? src.dev : src.host) = static_cast<const uint64_t*>(rows);
    return groth16_prove_batch_any(ctx, pk, rd, src, flags, r, s, count, proofs);
}
extern "C" int zl_groth16_prove_batch(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, const uint64_t* assignments, unsigned flags, const uint64_t* r,
                                      const uint64_t* s, size_t count, zl_g16_proof* proofs) {
    return groth16_prove_batch_rows(ctx, pk, r1cs_handle, assignments, false, flags, r, s, count, proofs);
}
extern "C" int zl_groth16_prove_batch_dev(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, const void* d_assignments, unsigned flags, const uint64_t* r,
                                          const uint64_t* s, size_t count, zl_g16_proof* proofs) {
    return groth16_prove_batch_rows(ctx, pk, r1cs_handle, d_assignments, true, flags, r, s, count, proofs);
}
extern "C" int zl_groth16_prove_poseidon_chains(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, uint32_t k, const uint64_t* x0, const uint64_t* x1, const uint64_t* r,
                                                const uint64_t* s, size_t count, zl_g16_proof* proofs, uint64_t* public_out) {
    const size_t nv = zl_poseidon_chain_assignment_elems(k);
    if (!ctx || !pk || nv == 0 || (count && (!x0 || !x1 || !r || !s || !proofs))) return ZL_EINVAL;
    const zl_r1cs_dev* rd = nullptr;
    const int rc0 = g16_entry(ctx, pk, r1cs_handle, r, s, count, &rd);
    if (rc0) return rc0;
    if (pk->curve != ZL_BLS12_381 && pk->curve != ZL_BN254) return ZL_EINVAL;
    // the shape of a k-link chain; what the matrices say cannot be checked, as with a witness-only compiler
    if (rd->n_instance != 2 || rd->n_witness != nv - 2 || rd->n_constraints != nv - 3) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    const zl_curve_t curve = pk->curve;
    G16BatchSource src;
    src.fill_dev = [=](size_t c0, size_t ch, void* d_rows) {
        return zl_poseidon_trace_rows(ctx, (int)curve, x0 + c0 * 4, x1 + c0 * 4, k, ch, d_rows, nv, public_out ? public_out + c0 * 4 : nullptr);
    };
    src.fill_host = [=](size_t c0, size_t ch, uint64_t* rows) {
        const int rc = zl_poseidon_chain_assignments(ctx, curve, x0 + c0 * 4, x1 + c0 * 4, k, ch, rows);
        if (rc == ZL_OK && public_out)
            for (size_t j = 0; j < ch; j++) memcpy(public_out + (c0 + j) * 4, rows + j * nv * 4 + 4, 32);
        return rc;
    };
    return groth16_prove_batch_any(ctx, pk, rd, src, 0, r, s, count, proofs);
}
// the checks the two membership provers share, in zl_groth16_prove_batch's order; *rd_out = the resident circuit
static int g16_merkle_checks(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, unsigned depth, bool args_ok, const uint64_t* r, const uint64_t* s, size_t count,
                             const zl_r1cs_dev** rd_out) {
    const size_t nv = zl_poseidon_merkle_assignment_elems(depth);
    if (!ctx || !pk || nv == 0 || !args_ok) return ZL_EINVAL;
    const zl_r1cs_dev* rd = nullptr;
    const int rc = g16_entry(ctx, pk, r1cs_handle, r, s, count, &rd);
    if (rc) return rc;
    if (pk->curve != ZL_BLS12_381 && pk->curve != ZL_BN254) return ZL_EINVAL;
    // the shape of a depth-d membership circuit; what the matrices say cannot be checked, as with a witness-only compiler
    if (rd->n_instance != 2 || rd->n_witness != nv - 2 || rd->n_constraints != nv - 2 - depth) return ZL_EINVAL;
    *rd_out = rd;
    return ZL_OK;
}
extern "C" int zl_groth16_prove_merkle_paths(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, unsigned depth, const uint64_t* leaves, const uint64_t* indices,
                                             const uint64_t* paths, const uint64_t* r, const uint64_t* s, size_t count, zl_g16_proof* proofs, uint64_t* roots_out) {
    const zl_r1cs_dev* rd = nullptr;
    const int rc0 = g16_merkle_checks(ctx, pk, r1cs_handle, depth, !(count && (!leaves || !indices || !paths || !r || !s || !proofs)), r, s, count, &rd);
    if (rc0) return rc0;
    for (size_t i = 0; i < count; i++)
        if (indices[i] >> depth) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    const size_t nv = zl_poseidon_merkle_assignment_elems(depth);
    const zl_curve_t curve = pk->curve;
    G16BatchSource src;
    src.fill_dev = [=](size_t c0, size_t ch, void* d_rows) {
        return zl_poseidon_merkle_trace_rows(ctx, (int)curve, leaves + c0 * 4, indices + c0, paths + c0 * depth * 4, depth, ch, d_rows, nv, roots_out ? roots_out + c0 * 4 : nullptr);
    };
    src.fill_host = [=](size_t c0, size_t ch, uint64_t* rows) {
        const int rc = zl_poseidon_merkle_assignments(ctx, curve, leaves + c0 * 4, indices + c0, paths + c0 * depth * 4, depth, ch, rows);
        if (rc == ZL_OK && roots_out)
            for (size_t j = 0; j < ch; j++) memcpy(roots_out + (c0 + j) * 4, rows + j * nv * 4 + 4, 32);
        return rc;
    };
    return groth16_prove_batch_any(ctx, pk, rd, src, 0, r, s, count, proofs);
}
extern "C" int zl_groth16_prove_merkle_members(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, const void* d_nodes, size_t n, unsigned depth, const uint64_t* indices,
                                               const uint64_t* r, const uint64_t* s, size_t count, zl_g16_proof* proofs, uint64_t* root_out) {
    const zl_r1cs_dev* rd = nullptr;
    const int rc0 = g16_merkle_checks(ctx, pk, r1cs_handle, depth, !(count && (!d_nodes || !indices || !r || !s || !proofs)), r, s, count, &rd);
    if (rc0) return rc0;
    if (zl_poseidon_merkle_nodes(n, depth) == 0 && n != 0) return ZL_EINVAL;  // (n > 2^depth)
    for (size_t i = 0; i < count; i++)
        if (indices[i] >= n) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    const size_t nv = zl_poseidon_merkle_assignment_elems(depth);
    const zl_curve_t curve = pk->curve;
    G16BatchSource src;
    src.fill_dev = [=](size_t c0, size_t ch, void* d_rows) { return zl_poseidon_merkle_member_rows(ctx, (int)curve, d_nodes, n, depth, indices + c0, ch, d_rows, nv, nullptr); };
    src.fill_host = [=](size_t c0, size_t ch, uint64_t* rows) { return zl_poseidon_merkle_member_rows(ctx, (int)curve, d_nodes, n, depth, indices + c0, ch, nullptr, nv, rows); };
    const int rc = groth16_prove_batch_any(ctx, pk, rd, src, 0, r, s, count, proofs);
    if (rc == ZL_OK && root_out) {  // the one root of the tree: the last node of the array
        ZL_HIP(ctx, hipMemcpyAsync(root_out, static_cast<const uint64_t*>(d_nodes) + (zl_poseidon_merkle_nodes(n, depth) - 1) * 4, 32, hipMemcpyDeviceToHost, ctx->stream));
        ZL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return rc;
}
// zl_groth16_prove_merkle_members with a tree per proof: the rows come out of a Merkle forest (ForestSrc of zl_poseidon_dev.hip), the roots with them
extern "C" int zl_groth16_prove_forest_members(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, const zl_merkle_forest* f, const uint32_t* tree_of,
                                               const uint64_t* indices, const uint64_t* r, const uint64_t* s, size_t count, zl_g16_proof* proofs, uint64_t* roots_out) {
    int fcurve = 0;
    unsigned depth = 0;
    if (zl_merkle_forest_prover_view(f, ctx, &fcurve, &depth)) return ZL_EINVAL;
    const zl_r1cs_dev* rd = nullptr;
    const int rc0 = g16_merkle_checks(ctx, pk, r1cs_handle, depth, !(count && (!tree_of || !indices || !r || !s || !proofs)), r, s, count, &rd);
    if (rc0) return rc0;
    if ((int)pk->curve != fcurve || zl_merkle_forest_members_ok(f, tree_of, indices, count)) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    const size_t nv = zl_poseidon_merkle_assignment_elems(depth);
    G16BatchSource src;
    src.fill_dev = [=](size_t c0, size_t ch, void* d_rows) {
        return zl_merkle_forest_member_rows(ctx, f, tree_of + c0, indices + c0, ch, d_rows, nv, nullptr, roots_out ? roots_out + c0 * 4 : nullptr);
    };
    src.fill_host = [=](size_t c0, size_t ch, uint64_t* rows) {
        return zl_merkle_forest_member_rows(ctx, f, tree_of + c0, indices + c0, ch, nullptr, nv, rows, roots_out ? roots_out + c0 * 4 : nullptr);
    };
    return groth16_prove_batch_any(ctx, pk, rd, src, 0, r, s, count, proofs);
}
// the checks the three arity-general provers share, in zl_groth16_prove_batch's order; nv = the row length of the stated (arity, depth), depth == 0 for the
// hash circuit; *rd_out = the resident circuit
static int g16_arity_checks(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, unsigned arity, size_t nv, unsigned depth, bool args_ok, const uint64_t* r,
                            const uint64_t* s, size_t count, const zl_r1cs_dev** rd_out) {
    if (!ctx || !pk || nv == 0 || !args_ok) return ZL_EINVAL;
    const zl_r1cs_dev* rd = nullptr;
    const int rc = g16_entry(ctx, pk, r1cs_handle, r, s, count, &rd);
    if (rc) return rc;
    if (pk->curve != ZL_BLS12_381 && pk->curve != ZL_BN254) return ZL_EINVAL;
    // the shape (2, a + 3 S(a) + 238 d, 3 S(a) + 237 d + 1) with nv = 2 + a + 3 S(a) + 238 d; what the matrices say cannot be checked, as with a witness-only compiler
    if (rd->n_instance != 2 || rd->n_witness != nv - 2 || rd->n_constraints != nv - 1 - arity - depth) return ZL_EINVAL;
    *rd_out = rd;
    return ZL_OK;
}
extern "C" int zl_groth16_prove_poseidon_hashes(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, unsigned arity, const uint64_t* in, const uint64_t* r,
                                                const uint64_t* s, size_t count, zl_g16_proof* proofs, uint64_t* public_out) {
    const size_t nv = zl_poseidon_hash_assignment_elems(arity);
    const zl_r1cs_dev* rd = nullptr;
    const int rc0 = g16_arity_checks(ctx, pk, r1cs_handle, arity, nv, 0, !(count && (!in || !r || !s || !proofs)), r, s, count, &rd);
    if (rc0 || count == 0) return rc0;
    const zl_curve_t curve = pk->curve;
    G16BatchSource src;
    src.fill_dev = [=](size_t c0, size_t ch, void* d_rows) {
        return zl_poseidon_hash_trace_rows(ctx, (int)curve, arity, in + c0 * arity * 4, ch, d_rows, nv, public_out ? public_out + c0 * 4 : nullptr);
    };
    src.fill_host = [=](size_t c0, size_t ch, uint64_t* rows) {
        const int rc = zl_poseidon_hash_assignments(ctx, curve, arity, in + c0 * arity * 4, ch, rows);
        if (rc == ZL_OK && public_out)
            for (size_t j = 0; j < ch; j++) memcpy(public_out + (c0 + j) * 4, rows + j * nv * 4 + 4, 32);
        return rc;
    };
    return groth16_prove_batch_any(ctx, pk, rd, src, 0, r, s, count, proofs);
}
extern "C" int zl_groth16_prove_merkle_leaf_paths(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, unsigned arity, unsigned depth, const uint64_t* preimages,
                                                  const uint64_t* indices, const uint64_t* paths, const uint64_t* r, const uint64_t* s, size_t count, zl_g16_proof* proofs,
                                                  uint64_t* roots_out) {
    const size_t nv = zl_poseidon_merkle_leaf_assignment_elems(arity, depth);
    const zl_r1cs_dev* rd = nullptr;
    const int rc0 = g16_arity_checks(ctx, pk, r1cs_handle, arity, nv, depth, !(count && (!preimages || !indices || !paths || !r || !s || !proofs)), r, s, count, &rd);
    if (rc0) return rc0;
    for (size_t i = 0; i < count; i++)
        if (indices[i] >> depth) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    const zl_curve_t curve = pk->curve;
    G16BatchSource src;
    src.fill_dev = [=](size_t c0, size_t ch, void* d_rows) {
        return zl_poseidon_merkle_leaf_trace_rows(ctx, (int)curve, arity, preimages + c0 * arity * 4, indices + c0, paths + c0 * depth * 4, depth, ch, d_rows, nv,
                                                  roots_out ? roots_out + c0 * 4 : nullptr);
    };
    src.fill_host = [=](size_t c0, size_t ch, uint64_t* rows) {
        const int rc = zl_poseidon_merkle_leaf_assignments(ctx, curve, arity, preimages + c0 * arity * 4, indices + c0, paths + c0 * depth * 4, depth, ch, rows);
        if (rc == ZL_OK && roots_out)
            for (size_t j = 0; j < ch; j++) memcpy(roots_out + (c0 + j) * 4, rows + j * nv * 4 + 4, 32);
        return rc;
    };
    return groth16_prove_batch_any(ctx, pk, rd, src, 0, r, s, count, proofs);
}
extern "C" int zl_groth16_prove_merkle_leaf_members(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, unsigned arity, const void* d_nodes, const void* d_preimages,
                                                    size_t n, unsigned depth, const uint64_t* indices, const uint64_t* r, const uint64_t* s, size_t count,
                                                    zl_g16_proof* proofs, uint64_t* root_out) {
    const size_t nv = zl_poseidon_merkle_leaf_assignment_elems(arity, depth);
    const zl_r1cs_dev* rd = nullptr;
    const int rc0 = g16_arity_checks(ctx, pk, r1cs_handle, arity, nv, depth, !(count && (!d_nodes || !d_preimages || !indices || !r || !s || !proofs)), r, s, count, &rd);
    if (rc0) return rc0;
    if (zl_poseidon_merkle_nodes(n, depth) == 0 && n != 0) return ZL_EINVAL;  // (n > 2^depth)
    for (size_t i = 0; i < count; i++)
        if (indices[i] >= n) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    const zl_curve_t curve = pk->curve;
    G16BatchSource src;
    src.fill_dev = [=](size_t c0, size_t ch, void* d_rows) {
        return zl_poseidon_merkle_leaf_member_rows(ctx, (int)curve, arity, d_nodes, d_preimages, n, depth, indices + c0, ch, d_rows, nv, nullptr);
    };
    src.fill_host = [=](size_t c0, size_t ch, uint64_t* rows) {
        return zl_poseidon_merkle_leaf_member_rows(ctx, (int)curve, arity, d_nodes, d_preimages, n, depth, indices + c0, ch, nullptr, nv, rows);
    };
    const int rc = groth16_prove_batch_any(ctx, pk, rd, src, 0, r, s, count, proofs);
    if (rc == ZL_OK && root_out) {  // the one root of the tree: the last node of the array
        ZL_HIP(ctx, hipMemcpyAsync(root_out, static_cast<const uint64_t*>(d_nodes) + (zl_poseidon_merkle_nodes(n, depth) - 1) * 4, 32, hipMemcpyDeviceToHost, ctx->stream));
        ZL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return rc;
}
// Encryptions from key, header and plaintext: the trace kernel writes each chunk's rows into the chunk's block; tag and ciphertext of every proof come out beside them
extern "C" int zl_groth16_prove_poseidon_encryptions(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, unsigned width, const uint64_t* initial_state,
                                                     const uint64_t* keys, size_t key_len, const uint64_t* headers, size_t header_len, const uint64_t* plaintexts, size_t blocks,
                                                     const uint64_t* r, const uint64_t* s, size_t count, zl_g16_proof* proofs, uint64_t* tags_out, uint64_t* ciphertexts_out) {
    const size_t nv = zl_poseidon_encrypt_assignment_elems(width, key_len, header_len, blocks);
    if (!ctx || !pk || nv == 0 || (count && (!keys || (header_len && !headers) || !plaintexts || !r || !s || !proofs))) return ZL_EINVAL;
    const zl_r1cs_dev* rd = nullptr;
    const int rc0 = g16_entry(ctx, pk, r1cs_handle, r, s, count, &rd);
    if (rc0) return rc0;
    if (pk->curve != ZL_BLS12_381 && pk->curve != ZL_BN254) return ZL_EINVAL;
    // the shape (2 + N rate + H, K + N rate + 3 S, 3 S + 1 + N rate) with nv = 2 + 2 N rate + H + K + 3 S; what the matrices say cannot be checked, as with a
    // witness-only compiler
    const size_t T = blocks * (width - 1), ni = 2 + T + header_len;
    if (rd->n_instance != ni || rd->n_witness != nv - ni || rd->n_constraints != nv - ni - key_len + 1) return ZL_EINVAL;
    const zl_curve_t curve = pk->curve;
    // initial_state is checked here, before any work and whatever the count (a call of no rows validates the parameters and writes nothing)
    const int rc1 = zl_poseidon_encrypt_assignments(nullptr, curve, width, initial_state, nullptr, key_len, nullptr, header_len, nullptr, blocks, 0, nullptr);
    if (rc1 || count == 0) return rc1;
    G16BatchSource src;
    src.fill_dev = [=](size_t c0, size_t ch, void* d_rows) {
        return zl_poseidon_encrypt_trace_rows(ctx, (int)curve, width, initial_state, keys + c0 * key_len * 4, key_len, headers + c0 * header_len * 4, header_len,
                                              plaintexts + c0 * T * 4, blocks, ch, d_rows, nv, tags_out ? tags_out + c0 * 4 : nullptr,
                                              ciphertexts_out ? ciphertexts_out + c0 * T * 4 : nullptr);
    };
    src.fill_host = [=](size_t c0, size_t ch, uint64_t* rows) {
        const int rc = zl_poseidon_encrypt_assignments(ctx, curve, width, initial_state, keys + c0 * key_len * 4, key_len, headers + c0 * header_len * 4, header_len,
                                                       plaintexts + c0 * T * 4, blocks, ch, rows);
        for (size_t j = 0; rc == ZL_OK && j < ch; j++) {
            if (tags_out) memcpy(tags_out + (c0 + j) * 4, rows + j * nv * 4 + 4, 32);
            if (ciphertexts_out) memcpy(ciphertexts_out + (c0 + j) * T * 4, rows + j * nv * 4 + 8, T * 32);
        }
        return rc;
    };
    return groth16_prove_batch_any(ctx, pk, rd, src, 0, r, s, count, proofs);
}
// Scalar multiplications on the embedded curve from point and scalar: the trace kernel writes each chunk's rows into the chunk's block, Q comes out beside them
extern "C" int zl_groth16_prove_ed_scalar_muls(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, unsigned bits, const uint64_t* points_xy, size_t point_stride,
                                               const uint64_t* scalars, const uint64_t* r, const uint64_t* s, size_t count, zl_g16_proof* proofs, uint64_t* results_out) {
    if (!ctx || !pk || point_stride > 1 || (count && (!points_xy || !scalars || !r || !s || !proofs))) return ZL_EINVAL;
    const zl_r1cs_dev* rd = nullptr;
    const int rc0 = g16_entry(ctx, pk, r1cs_handle, r, s, count, &rd);
    if (rc0) return rc0;
    const zl_curve_t curve = pk->curve;
    const size_t nv = zl_ed_scalar_mul_assignment_elems(curve, bits);  // (0 for an unknown curve as well)
    // the shape (5, 14 bits - 10, 14 bits - 8) with nv = 14 bits - 5; what the matrices say cannot be checked, as with a witness-only compiler
    if (nv == 0 || rd->n_instance != 5 || rd->n_witness != nv - 5 || rd->n_constraints != nv - 3) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    G16BatchSource src;
    src.fill_dev = [=](size_t c0, size_t ch, void* d_rows) {
        return zl_ed_scalar_mul_trace_rows(ctx, (int)curve, bits, points_xy + c0 * point_stride * 8, point_stride, scalars + c0 * 4, ch, d_rows, nv,
                                           results_out ? results_out + c0 * 8 : nullptr);
    };
    src.fill_host = [=](size_t c0, size_t ch, uint64_t* rows) {
        const int rc = zl_ed_scalar_mul_assignments(ctx, curve, bits, points_xy + c0 * point_stride * 8, point_stride, scalars + c0 * 4, ch, rows);
        for (size_t j = 0; rc == ZL_OK && results_out && j < ch; j++) memcpy(results_out + (c0 + j) * 8, rows + j * nv * 4 + 12, 64);
        return rc;
    };
    return groth16_prove_batch_any(ctx, pk, rd, src, 0, r, s, count, proofs);
}
// Hybrid encryptions from generator, ephemeral keys, public keys, headers and plaintexts: the ladder launch and the cipher launch write each chunk's rows into
// the chunk's block; epk, tag and ciphertext come out beside the proofs.  The agreement and the cipher run once.
extern "C" int zl_groth16_prove_hybrid_encryptions(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, unsigned width, unsigned bits, const uint64_t* initial_state,
                                                   const uint64_t* generator_xy, const uint64_t* esk, const uint64_t* pks_xy, size_t pk_stride, const uint64_t* headers,
                                                   size_t header_len, const uint64_t* plaintexts, size_t blocks, const uint64_t* r, const uint64_t* s, size_t count,
                                                   zl_g16_proof* proofs, uint64_t* epks_out, uint64_t* tags_out, uint64_t* ciphertexts_out) {
    if (!ctx || !pk || !generator_xy || pk_stride > 1 || (count && (!esk || !pks_xy || (header_len && !headers) || !plaintexts || !r || !s || !proofs))) return ZL_EINVAL;
    const zl_r1cs_dev* rd = nullptr;
    const int rc0 = g16_entry(ctx, pk, r1cs_handle, r, s, count, &rd);
    if (rc0) return rc0;
    const zl_curve_t curve = pk->curve;
    const size_t nv = zl_hybrid_encrypt_assignment_elems(curve, width, bits, header_len, blocks);  // (0 for an unknown curve as well)
    if (nv == 0) return ZL_EINVAL;
    // the shape: n_instance = 8 + T + H fixes where the witnesses begin, n_witness = nv - n_instance, and the family's n_witness - (n_constraints - 1) = -2; what
    // the matrices say cannot be checked, as with a witness-only compiler
    const size_t T = blocks * (width - 1), ni = 8 + T + header_len;
    if (rd->n_instance != ni || rd->n_witness != nv - ni || rd->n_constraints != rd->n_witness + 3) return ZL_EINVAL;
    // the initial state and the generator, before any work (and at count == 0)
    const int rc1 = zl_hybrid_encrypt_assignments(nullptr, curve, width, bits, initial_state, generator_xy, nullptr, nullptr, 0, nullptr, header_len, nullptr, blocks, 0, nullptr);
    if (rc1) return rc1;
    if (count == 0) return ZL_OK;
    const size_t H = header_len;
    G16BatchSource src;
    src.fill_dev = [=](size_t c0, size_t ch, void* d_rows) {
        return zl_hybrid_encrypt_trace_rows(ctx, (int)curve, width, bits, initial_state, generator_xy, esk + c0 * 4, pks_xy + c0 * pk_stride * 8, pk_stride, headers + c0 * H * 4, H,
                                            plaintexts + c0 * T * 4, blocks, ch, d_rows, nv, epks_out ? epks_out + c0 * 8 : nullptr, tags_out ? tags_out + c0 * 4 : nullptr,
                                            ciphertexts_out ? ciphertexts_out + c0 * T * 4 : nullptr);
    };
    src.fill_host = [=](size_t c0, size_t ch, uint64_t* rows) {
        const int rc = zl_hybrid_encrypt_assignments(ctx, curve, width, bits, initial_state, generator_xy, esk + c0 * 4, pks_xy + c0 * pk_stride * 8, pk_stride, headers + c0 * H * 4,
                                                     H, plaintexts + c0 * T * 4, blocks, ch, rows);
        for (size_t j = 0; rc == ZL_OK && j < ch; j++) {  // [5..7) epk, [7] tag, [8 .. 8 + T) ciphertext
            const uint64_t* row = rows + j * nv * 4;
            if (epks_out) memcpy(epks_out + (c0 + j) * 8, row + 20, 64);
            if (tags_out) memcpy(tags_out + (c0 + j) * 4, row + 28, 32);
            if (ciphertexts_out) memcpy(ciphertexts_out + (c0 + j) * T * 4, row + 32, T * 32);
        }
        return rc;
    };
    return groth16_prove_batch_any(ctx, pk, rd, src, 0, r, s, count, proofs);
}
extern "C" int zl_groth16_last_h(zl_ctx* ctx, uint64_t* out, size_t n) {
    if (!ctx || !out || !ctx->g16_h || n > ctx->g16_h_n) return ZL_EINVAL;
    ZL_HIP(ctx, hipMemcpyAsync(out, ctx->g16_h, n * 32, hipMemcpyDeviceToHost, ctx->stream));
    ZL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZL_OK;
}
