// zl_msm_multi_plan.h -- host side of zl_msm_multi_dev that needs neither a ctx nor a device: the argument checks and the planner that cuts
// `count` scalar vectors into chunks whose slice partials fit the scratch slot.  Plain C++ (no HIP): zl_msm_multi.hip includes it, and so does the
// stand-alone sanitizer program tests/c/msm_multi_host.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define ZL_MM_C 6            // window width: unsigned digits 1..63, one bucket per lane of a wave (digit 0 is skipped, lane 0 idles in the walk)
#define ZL_MM_WINDOWS 43     // ceil(256 / 6): every bit of the 32-byte scalar is covered, the top window holds 4 bits
#define ZL_MM_SLICE 2048     // points per workgroup at most: digits (u8) and the sorted index list (u16) of a slice live in LDS
#define ZL_MM_MAX_CHUNK 65535  // vectors per launch: the chunk is the grid's z extent
// Scratch budget of ZL_SLOT_MSM_MULTI: it bounds how many vectors share a launch chain, NOT the size of one vector.  A chunk holds at least one vector, and
// a vector of n points always needs 43 * ceil(n / 2048) partial sums (79 MB at 2^24 points on BLS12-381 G1, tens of GB near 2^31): beyond ~2^20 points the
// slot grows past the budget and the call is the wrong tool anyway (zl_msm_dev's wide windows do half the additions there).
#define ZL_MM_BUDGET ((size_t)256 << 20)

struct zl_mm_plan {
    uint32_t slices = 0;     // point slices per vector
    uint32_t slice_len = 0;  // points per slice (the last one may be shorter)
    size_t per_vector = 0;   // scratch bytes per vector
    size_t chunk = 0;        // vectors per launch chain
    size_t chunks = 0;       // launch chains of the call
};

// Where the pieces of one chunk lie in the scratch block (byte offsets; every piece holds plan.chunk records).  The driver carves the block with this and
// nothing else; tests/c/msm_multi_host.cpp walks a host mock of the block through the same offsets.
struct zl_mm_layout {
    size_t bad = 0;      // u32 flag: a scalar with bits above the field's width was seen
    size_t part = 0;     // XYZZ[chunk][ZL_MM_WINDOWS][slices]: the slice sums; index of (v, w, s) = (v * ZL_MM_WINDOWS + w) * slices + s
    size_t res = 0;      // XYZZ[chunk]: the Horner results
    size_t aff = 0;      // Affine[chunk]
    size_t prefix = 0;   // F[chunk]: running products of the batch inversion
    size_t words = 0;    // canonical x || y words [chunk]
    size_t total = 0;    // bytes of the block
};
// point_bytes = sizeof(XYZZ<F>), affine_bytes = sizeof(Affine<F>), field_bytes = sizeof(F), out_bytes = canonical words of one result
inline size_t zl_mm_stage_bytes(size_t point_bytes, size_t affine_bytes, size_t field_bytes, size_t out_bytes) { return point_bytes + affine_bytes + field_bytes + out_bytes; }
inline zl_mm_layout zl_mm_make_layout(const zl_mm_plan& p, size_t point_bytes, size_t affine_bytes, size_t field_bytes, size_t out_bytes) {
    zl_mm_layout l;
    l.bad = 0;
    l.part = 64;
    l.res = l.part + p.chunk * ZL_MM_WINDOWS * p.slices * point_bytes;
    l.aff = l.res + p.chunk * point_bytes;
    l.prefix = l.aff + p.chunk * affine_bytes;
    l.words = l.prefix + p.chunk * field_bytes;
    l.total = l.words + p.chunk * out_bytes;  // = 64 + chunk * per_vector when the plan was made with zl_mm_stage_bytes of the same sizes
    return l;
}

// the ABI's checks of zl_msm_multi_dev once the handle has been found (bases_n = points of the handle): ZL_OK = 0, ZL_EINVAL = -1
inline int zl_mm_check_args(size_t bases_n, size_t first, const void* d_scalars, size_t n, size_t stride_scalars, size_t count, const uint64_t* out_xy) {
    if (first > bases_n || n > bases_n - first) return -1;
    if (n > 0x7fffffffu) return -1;
    if (count == 0) return 0;
    if (!out_xy) return -1;
    if (n == 0) return 0;
    if (!d_scalars || stride_scalars < n) return -1;
    if (count > 1 && stride_scalars > (SIZE_MAX / 32) / (count - 1)) return -1;  // the last vector's address must not wrap
    return 0;
}

// point_bytes = sizeof(XYZZ<F>) of the group, stage_bytes = the per-vector result staging (zl_mm_stage_bytes).
// chunk_override > 0 (ZL_TUNE_MSM_MULTI_CHUNK) replaces the chunk the budget gives; both are clamped to [1, min(count, ZL_MM_MAX_CHUNK)].
inline zl_mm_plan zl_mm_make_plan(size_t n, size_t count, size_t point_bytes, size_t stage_bytes, size_t budget, long chunk_override) {
    zl_mm_plan p;
    if (n == 0 || count == 0) return p;
    p.slices = (uint32_t)((n + ZL_MM_SLICE - 1) / ZL_MM_SLICE);
    p.slice_len = (uint32_t)((n + p.slices - 1) / p.slices);
    p.per_vector = (size_t)ZL_MM_WINDOWS * p.slices * point_bytes + stage_bytes;
    size_t chunk = budget / p.per_vector;
    if (chunk_override > 0) chunk = (size_t)chunk_override;
    if (chunk < 1) chunk = 1;
    if (chunk > ZL_MM_MAX_CHUNK) chunk = ZL_MM_MAX_CHUNK;
    if (chunk > count) chunk = count;
    p.chunk = chunk;
    p.chunks = (count + chunk - 1) / chunk;
    return p;
}
