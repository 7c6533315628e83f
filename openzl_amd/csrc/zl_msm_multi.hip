// zl_msm_multi.hip -- `count` MSMs over ONE base range in one device pass (zl_msm_multi_dev), for one group: -DZL_G=BlsG1|BnG1|BlsG2|BnG2.
//
// The single MSM (zl_msm.hip) spends a sort / accumulate / tail launch chain per scalar vector and sizes its windows for millions of points.  A batch
// of small vectors over one key has the opposite shape: few points, many vectors.  Here the batch is the parallel dimension:
//   k_mm_accumulate  one wave per (vector, window, point slice).  Windows are ZL_MM_C = 6 bits wide, so the wave owns the whole bucket set of its
//                    window: bucket d belongs to lane d.  The digits of the slice are counting-sorted in LDS; the lanes then walk their own lists in
//                    lockstep (one mixed addition per lane and step, for every lane that still has an entry).  sum_d d B_d is a lane-to-lane suffix
//                    scan (S_d = sum_{k >= d} B_k) followed by a tree over S_1..S_63, the operands exchanged through LDS.
//   k_mm_fold        one lane per (vector, window): adds the slices (only when a vector has more than one).
//   k_mm_horner      one lane per vector: Horner over the 43 windows, six doublings per window.
//   k_batch_affine, k_bases_export (zl_msm_bases.h): canonical affine words, exactly the bytes zl_msm_dev returns.
// The result is a group element in canonical affine form, so it does not depend on the window width, the slice cut or the order inside a bucket.
// Bases at infinity (the handle's d_inf) and zero digits never reach a bucket; the additions are the complete ones of zl_curve.h (P + P, P - P, infinity).
// A handle's window table (zl_bases_precompute) is built for windows of 16 bits and more and is not used: both kinds of handle take this path.
#include <string.h>
#include <algorithm>
#include "zl_ctx.h"
#include "zl_msm_common.h"
#include "zl_msm_bases.h"
#include "zl_msm_multi_plan.h"

#ifndef ZL_G
#error "compile with -DZL_G=<group config>"
#endif

template <class F> __device__ __noinline__ void zl_mm_dbl_window_ool(XYZZ<F>* p) { zl::dbl_n(*p, ZL_MM_C); }

template <class G>
__global__ void __launch_bounds__(64) k_mm_accumulate(const Affine<typename G::F>* __restrict__ bases, const uint8_t* __restrict__ inf, const uint32_t* __restrict__ scalars,
                                                       size_t stride_words, uint32_t n, uint32_t slice_len, XYZZ<typename G::F>* __restrict__ out, uint32_t* __restrict__ bad) {
    using F = typename G::F;
    using X = XYZZ<F>;
    __shared__ uint8_t dig[ZL_MM_SLICE];
    __shared__ uint16_t list[ZL_MM_SLICE];
    __shared__ uint32_t cnt[64];
    __shared__ __attribute__((aligned(16))) uint32_t xch_raw[64 * sizeof(X) / 4];
    X* xch = reinterpret_cast<X*>(xch_raw);
    const uint32_t lane = threadIdx.x, s = blockIdx.x, w = blockIdx.y, v = blockIdx.z;
    const size_t base0 = (size_t)s * slice_len;
    const uint32_t m = base0 >= n ? 0u : n - base0 < slice_len ? (uint32_t)(n - base0) : slice_len;  // m <= ZL_MM_SLICE (zl_mm_make_plan)
    const uint32_t* sv = scalars + (size_t)v * stride_words + base0 * 8;
    const int word = (int)(w * ZL_MM_C) >> 5, sh = (int)(w * ZL_MM_C) & 31;
    cnt[lane] = 0;
    __syncthreads();
    for (uint32_t k = lane; k < m; k += 64) {
        const uint32_t* sc = sv + (size_t)k * 8;
        uint64_t x = sc[word];
        if (word < 7) x |= (uint64_t)sc[word + 1] << 32;
        uint32_t d = (uint32_t)(x >> sh) & ((1u << ZL_MM_C) - 1u);
        if (w == 0) zl_flag_wide_scalar(sc[7], G::SC_BITS, bad);
        if (inf && inf[base0 + k]) d = 0;
        dig[k] = (uint8_t)d;
        if (d) atomicAdd(&cnt[d], 1u);
    }
    __syncthreads();
    const uint32_t len = cnt[lane];
    uint32_t off = 0;
    for (uint32_t j = 0; j < lane; j++) off += cnt[j];
    __syncthreads();
    cnt[lane] = off;  // now the write cursor of bucket `lane`
    __syncthreads();
    for (uint32_t k = lane; k < m; k += 64) {
        const uint32_t d = dig[k];
        if (d) list[atomicAdd(&cnt[d], 1u)] = (uint16_t)k;
    }
    __syncthreads();
    X acc = X::inf();
    for (uint32_t t = 0; __any(t < len); t++) {
        if (t < len) {
            const Affine<F> P = bases[base0 + list[off + t]];
            zl::add_mixed(acc, P.x, P.y, false);
        }
    }
    // steps 0..5: suffix scan, lane d += lane d + 2^step; lane 0 (S_0 = S_1: bucket 0 is empty) then drops out; steps 6..11: tree over S_1..S_63
#pragma nounroll
    for (int step = 0; step < 12; step++) {
        if (step == 6 && lane == 0) acc = X::inf();
        const uint32_t o = 1u << (step < 6 ? step : step - 6);
        const bool take = step < 6 ? lane + o < 64 : (lane & (2 * o - 1)) == 0;
        xch[lane] = acc;
        __syncthreads();
        if (take) {
            const X q = xch[lane + o];
            zl::add_full(acc, q);
        }
        __syncthreads();
    }
    if (lane == 0) out[((size_t)v * ZL_MM_WINDOWS + w) * gridDim.x + s] = acc;
}

// part[i * slices] += part[i * slices + 1 ..]: one lane per (vector, window)
template <class G>
__global__ void __launch_bounds__(64) k_mm_fold(XYZZ<typename G::F>* __restrict__ part, uint32_t total, uint32_t slices) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    XYZZ<typename G::F>* p = part + (size_t)i * slices;
    XYZZ<typename G::F> acc = p[0];
    for (uint32_t s = 1; s < slices; s++) zl_add_full_ool(&acc, p + s);
    p[0] = acc;
}
// res[v] = sum_w 2^(6 w) part[(v W + w) slices]: one lane per vector
template <class G>
__global__ void __launch_bounds__(64) k_mm_horner(const XYZZ<typename G::F>* __restrict__ part, uint32_t count, uint32_t slices, XYZZ<typename G::F>* __restrict__ res) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= count) return;
    XYZZ<typename G::F> acc = XYZZ<typename G::F>::inf();
#pragma nounroll
    for (int w = ZL_MM_WINDOWS - 1; w >= 0; w--) {
        zl_mm_dbl_window_ool(&acc);
        zl_add_full_ool(&acc, part + ((size_t)v * ZL_MM_WINDOWS + w) * slices);
    }
    res[v] = acc;
}

template <class G>
static int msm_multi_t(zl_ctx* ctx, const zl_bases& bs, size_t first, const void* d_scalars, size_t n, size_t stride_scalars, size_t count, uint64_t* out_xy,
                       uint8_t* out_inf) {
    using F = typename G::F;
    using X = XYZZ<F>;
    constexpr int WORDS = FieldIO<F>::WORDS;
    constexpr size_t OUT_BYTES = (size_t)2 * WORDS * 4;  // canonical x || y of one result
    static_assert(sizeof(X) % 16 == 0 && sizeof(F) % 8 == 0, "scratch carving below");
    int rc = zl_mm_check_args(bs.n, first, d_scalars, n, stride_scalars, count, out_xy);
    if (rc) return rc;
    if (count == 0) return ZL_OK;
    if (n == 0) {
        memset(out_xy, 0, count * OUT_BYTES);
        if (out_inf) memset(out_inf, 1, count);
        return ZL_OK;
    }
    const zl_mm_plan plan = zl_mm_make_plan(n, count, sizeof(X), zl_mm_stage_bytes(sizeof(X), sizeof(Affine<F>), sizeof(F), OUT_BYTES), ZL_MM_BUDGET,
                                            zl_tune("ZL_TUNE_MSM_MULTI_CHUNK", 0));
    const zl_mm_layout lay = zl_mm_make_layout(plan, sizeof(X), sizeof(Affine<F>), sizeof(F), OUT_BYTES);
    void* d_block = nullptr;
    if ((rc = zl_scratch_get(ctx, ZL_SLOT_MSM_MULTI, lay.total, &d_block))) return rc;
    unsigned char* p = reinterpret_cast<unsigned char*>(d_block);
    uint32_t* d_bad = reinterpret_cast<uint32_t*>(p + lay.bad);
    X* d_part = reinterpret_cast<X*>(p + lay.part);
    X* d_res = reinterpret_cast<X*>(p + lay.res);
    Affine<F>* d_aff = reinterpret_cast<Affine<F>*>(p + lay.aff);
    F* d_prefix = reinterpret_cast<F*>(p + lay.prefix);
    uint32_t* d_words = reinterpret_cast<uint32_t*>(p + lay.words);

    hipStream_t st = ctx->stream;
    ctx->timing = zl_timing{};
    ZL_HIP(ctx, hipMemsetAsync(d_bad, 0, 4, st));
    const Affine<F>* d_bases = reinterpret_cast<const Affine<F>*>(bs.d_pts) + first;
    const uint8_t* d_inf = bs.d_inf ? reinterpret_cast<const uint8_t*>(bs.d_inf) + first : nullptr;
    for (size_t c0 = 0; c0 < count; c0 += plan.chunk) {
        const uint32_t ch = (uint32_t)std::min(plan.chunk, count - c0);
        const uint32_t* sc = reinterpret_cast<const uint32_t*>(d_scalars) + c0 * stride_scalars * 8;
        hipLaunchKernelGGL((k_mm_accumulate<G>), dim3(plan.slices, ZL_MM_WINDOWS, ch), dim3(64), 0, st, d_bases, d_inf, sc, stride_scalars * 8, (uint32_t)n, plan.slice_len,
                           d_part, d_bad);
        ZL_HIP(ctx, hipGetLastError());
        if (plan.slices > 1) {
            const uint32_t total = ch * ZL_MM_WINDOWS;
            hipLaunchKernelGGL((k_mm_fold<G>), dim3((total + 63) / 64), dim3(64), 0, st, d_part, total, plan.slices);
            ZL_HIP(ctx, hipGetLastError());
        }
        hipLaunchKernelGGL((k_mm_horner<G>), dim3((ch + 63) / 64), dim3(64), 0, st, d_part, ch, plan.slices, d_res);
        ZL_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL((k_batch_affine<G, 0>), dim3((ch + 63) / 64), dim3(64), 0, st, (const void*)d_res, ch, ch, d_prefix, d_aff);
        ZL_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL((k_bases_export<G>), dim3((ch + 127) / 128), dim3(128), 0, st, (const Affine<F>*)d_aff, ch, d_words);
        ZL_HIP(ctx, hipGetLastError());
        ZL_HIP(ctx, hipMemcpyAsync(reinterpret_cast<unsigned char*>(out_xy) + c0 * OUT_BYTES, d_words, ch * OUT_BYTES, hipMemcpyDeviceToHost, st));
        ctx->timing.launches++;  // per chunk: one launch of the dominant kernel (k_mm_accumulate), zl_timing's meaning of the field
    }
    uint32_t bad = 0;
    ZL_HIP(ctx, hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st));
    ZL_HIP(ctx, hipStreamSynchronize(st));
    ctx->timing.window_bits = ZL_MM_C;
    ctx->timing.entries = (uint64_t)count * n * ZL_MM_WINDOWS;
    if (bad) return ZL_EINVAL;  // a scalar with bits at or above SC_BITS, as in zl_msm_dev
    if (out_inf) {
        const uint32_t* wds = reinterpret_cast<const uint32_t*>(out_xy);
        for (size_t j = 0; j < count; j++) {
            uint32_t any = 0;
            for (int k = 0; k < 2 * WORDS; k++) any |= wds[j * 2 * WORDS + k];
            out_inf[j] = any ? 0 : 1;
        }
    }
    return ZL_OK;
}

int ZL_GNAME(zl_msm_multi_run)(zl_ctx* ctx, const zl_bases& b, size_t first, const void* d_scalars, size_t n, size_t stride_scalars, size_t count, uint64_t* out_xy,
                               uint8_t* out_inf) {
    return msm_multi_t<ZL_G>(ctx, b, first, d_scalars, n, stride_scalars, count, out_xy, out_inf);
}
