// zl_decode_dev.hip -- arkworks-compressed points and Groth16 proofs decoded on the device: the square root(s) for y, the sign rule and the subgroup
// check of ark-ec's deserializer (zl_serialize.h on the host, one record at a time), here one lane per point over a whole batch.
// Compiled once per curve (ZL_DECODE_CURVE = 1 BLS12-381, 2 BN254).  The arithmetic is zl_decode.h, shared with the host test hook.
//
// Kernels:
//   k_dec_g1 / k_dec_g2  one lane per point, one launch per group (a wave never mixes groups).  A lane reads its record bytewise from the packed input (record
//                        p of the first n_a points at p stride + off_a, of the others at (p - n_a) stride + off_b: plain points are one segment, a proof batch
//                        takes its A's and C's in one G1 launch), decodes it and writes canonical affine u64 words, an inf byte and an int32 status.
//                        Lanes at or above the point count return at once and write nothing.
//   k_dec_fq2_sqrt       test hook: fq2_sqrt of one canonical Fq2 value per lane.
// Plain Fp<Fq> / Fp2<Fq> (32-bit limbs, fully reduced) as in zl_pairing_dev.hip: nothing new for zl_bounds.h.  Every loop bound is a compile-time constant
// or a launch argument; a malformed, off-curve or non-subgroup record changes the status its lane writes, not the path it walks (zl_decode.h).
#include <string.h>
#include <memory>
#include <new>
#include "zl_ctx.h"
#include "zl_decode.h"
#include "zl_decode_dev.h"

#if ZL_DECODE_CURVE == 1
#define ZL_DD_DECODER openzl::decode::BlsDecoder
#define ZL_DD_SUFFIX(x) x##_bls
#else
#define ZL_DD_DECODER openzl::decode::BnDecoder
#define ZL_DD_SUFFIX(x) x##_bn
#endif

namespace {
using D = ZL_DD_DECODER;
using F = D::F;
using F2 = D::F2;
constexpr int NW = D::N;                                          // u32 words per Fq
constexpr size_t W1 = D::G1_WORDS64, W2 = D::G2_WORDS64;          // u64 words per decoded point
constexpr size_t B1 = D::G1_BYTES, B2 = D::G2_BYTES, PB = 2 * B1 + B2;  // bytes per compressed point / proof

__device__ __forceinline__ const uint8_t* record(const uint8_t* in, size_t p, size_t n_a, size_t stride, size_t off_a, size_t off_b) {
    return p < n_a ? in + p * stride + off_a : in + (p - n_a) * stride + off_b;
}
__global__ __launch_bounds__(64) void k_dec_g1(const uint8_t* __restrict__ in, size_t n_a, size_t n, size_t stride, size_t off_a, size_t off_b,
                                               uint64_t* __restrict__ out_xy, uint8_t* __restrict__ out_inf, int32_t* __restrict__ status) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    uint8_t inf;
    status[p] = D::decode_g1(record(in, p, n_a, stride, off_a, off_b), out_xy + p * W1, &inf);
    out_inf[p] = inf;
}
__global__ __launch_bounds__(64) void k_dec_g2(const uint8_t* __restrict__ in, size_t n_a, size_t n, size_t stride, size_t off_a, size_t off_b,
                                               uint64_t* __restrict__ out_xy, uint8_t* __restrict__ out_inf, int32_t* __restrict__ status) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    uint8_t inf;
    status[p] = D::decode_g2(record(in, p, n_a, stride, off_a, off_b), out_xy + p * W2, &inf);
    out_inf[p] = inf;
}

ZL_HD F load_canon64(const uint64_t* w) {  // canonical u64 words -> Montgomery
    F c;
#pragma unroll
    for (int i = 0; i < NW / 2; i++) {
        c.l[2 * i] = (uint32_t)w[i];
        c.l[2 * i + 1] = (uint32_t)(w[i] >> 32);
    }
    return zl::to_mont(c);
}
ZL_HD void fq2_sqrt_one(const uint64_t* in, uint64_t* out, uint8_t* ok) {
    const F2 a{load_canon64(in), load_canon64(in + NW / 2)};
    F2 r;
    const bool good = openzl::decode::fq2_sqrt(a, &r);
    const F2 rc = zl::from_mont(r);
    D::store64(out, rc.c0, good);
    D::store64(out + NW / 2, rc.c1, good);
    *ok = good ? 1 : 0;
}
__global__ __launch_bounds__(64) void k_dec_fq2_sqrt(const uint64_t* __restrict__ in, size_t n, uint64_t* __restrict__ out, uint8_t* __restrict__ ok) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    uint8_t good;
    fq2_sqrt_one(in + p * NW, out + p * NW, &good);
    ok[p] = good;
}

constexpr size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// the output block of one launch set in ZL_SLOT_DECODE_OUT: n1 G1 points, then n2 G2 points; words | statuses | inf bytes
struct OutLayout {
    size_t xy1, xy2, st1, st2, inf1, inf2, bytes;
    OutLayout(size_t n1, size_t n2) {
        xy1 = 0;
        xy2 = xy1 + up256(n1 * W1 * 8);
        st1 = xy2 + up256(n2 * W2 * 8);
        st2 = st1 + up256(n1 * 4);
        inf1 = st2 + up256(n2 * 4);
        inf2 = inf1 + up256(n1);
        bytes = inf2 + up256(n2);
    }
};

// upload `in_bytes` of records, decode n1 G1 points (segments of n1a and n1 - n1a) and n2 G2 points from them, download the whole output block into `host`
// (L.bytes).  Both copies move pageable memory (the caller's bytes, a plain host buffer): the runtime stages them, and the stream is drained before `host` is read.
int run(zl_ctx* ctx, const uint8_t* in, size_t in_bytes, size_t stride, size_t n1a, size_t n1, size_t off1a, size_t off1b, size_t n2, size_t off2,
        const OutLayout& L, unsigned char* host) {
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    void *d_in = nullptr, *d_out = nullptr;
    int rc = zl_scratch_get(ctx, ZL_SLOT_DECODE_IN, up256(in_bytes), &d_in);
    if (!rc) rc = zl_scratch_get(ctx, ZL_SLOT_DECODE_OUT, L.bytes, &d_out);
    if (rc) return rc;
    const uint8_t* din = static_cast<const uint8_t*>(d_in);
    unsigned char* dout = static_cast<unsigned char*>(d_out);
    ZL_HIP(ctx, hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (n2) {  // the long kernel first
        hipLaunchKernelGGL(k_dec_g2, dim3((unsigned)((n2 + 63) / 64)), dim3(64), 0, ctx->stream, din, n2, n2, stride, off2, off2,
                           reinterpret_cast<uint64_t*>(dout + L.xy2), dout + L.inf2, reinterpret_cast<int32_t*>(dout + L.st2));
        ZL_HIP(ctx, hipGetLastError());
    }
    if (n1) {
        hipLaunchKernelGGL(k_dec_g1, dim3((unsigned)((n1 + 63) / 64)), dim3(64), 0, ctx->stream, din, n1a, n1, stride, off1a, off1b,
                           reinterpret_cast<uint64_t*>(dout + L.xy1), dout + L.inf1, reinterpret_cast<int32_t*>(dout + L.st1));
        ZL_HIP(ctx, hipGetLastError());
    }
    ZL_HIP(ctx, hipMemcpyAsync(host, dout, L.bytes, hipMemcpyDeviceToHost, ctx->stream));
    ZL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZL_OK;
}
}  // namespace

namespace openzl {
namespace decode_dev {
int ZL_DD_SUFFIX(points)(zl_ctx* ctx, zl_group_t group, const uint8_t* in, size_t count, uint64_t* out_xy, uint8_t* out_inf, int32_t* status) {
    if (!ctx || (group != ZL_G1 && group != ZL_G2) || (count && (!in || !out_xy || !out_inf || !status))) return ZL_EINVAL;
    const bool g2 = group == ZL_G2;
    const size_t rec = g2 ? B2 : B1, words = g2 ? W2 : W1;
    const size_t m_max = count < MAX_RECORDS ? count : MAX_RECORDS;  // the first chunk is the largest: one host block, not zero-filled, for all of them
    const std::unique_ptr<unsigned char[]> host(new (std::nothrow) unsigned char[OutLayout(g2 ? 0 : m_max, g2 ? m_max : 0).bytes + 1]);
    if (!host) return ZL_ENOMEM;
    for (size_t first = 0; first < count; first += MAX_RECORDS) {
        const size_t m = count - first < MAX_RECORDS ? count - first : MAX_RECORDS;
        const OutLayout L(g2 ? 0 : m, g2 ? m : 0);
        const int rc = run(ctx, in + first * rec, m * rec, rec, g2 ? 0 : m, g2 ? 0 : m, 0, 0, g2 ? m : 0, 0, L, host.get());
        if (rc) return rc;
        memcpy(out_xy + first * words, host.get() + (g2 ? L.xy2 : L.xy1), m * words * 8);
        memcpy(status + first, host.get() + (g2 ? L.st2 : L.st1), m * 4);
        memcpy(out_inf + first, host.get() + (g2 ? L.inf2 : L.inf1), m);
    }
    return ZL_OK;
}
int ZL_DD_SUFFIX(proofs)(zl_ctx* ctx, const uint8_t* in, size_t count, zl_g16_proof* proofs, int32_t* status) {
    if (!ctx || (count && (!in || !proofs || !status))) return ZL_EINVAL;
    const size_t m_max = count < MAX_RECORDS ? count : MAX_RECORDS;
    const std::unique_ptr<unsigned char[]> host_block(new (std::nothrow) unsigned char[OutLayout(2 * m_max, m_max).bytes + 1]);
    if (!host_block) return ZL_ENOMEM;
    unsigned char* const host = host_block.get();
    for (size_t first = 0; first < count; first += MAX_RECORDS) {
        const size_t m = count - first < MAX_RECORDS ? count - first : MAX_RECORDS;
        const OutLayout L(2 * m, m);  // G1 points: the m A's, then the m C's
        const int rc = run(ctx, in + first * PB, m * PB, PB, m, 2 * m, 0, B1 + B2, m, B1, L, host);
        if (rc) return rc;
        const uint64_t* xy1 = reinterpret_cast<const uint64_t*>(host + L.xy1);
        const uint64_t* xy2 = reinterpret_cast<const uint64_t*>(host + L.xy2);
        const int32_t* st1 = reinterpret_cast<const int32_t*>(host + L.st1);
        const int32_t* st2 = reinterpret_cast<const int32_t*>(host + L.st2);
        const unsigned char *inf1 = host + L.inf1, *inf2 = host + L.inf2;
        for (size_t i = 0; i < m; i++) {
            // as zl_groth16_proof_from_bytes: the first failing point of A, B, C gives the status and ends the record; the points in front of it stay
            // decoded, the failing one and those behind it are zero
            zl_g16_proof& pr = proofs[first + i];
            memset(&pr, 0, sizeof pr);
            int32_t st = st1[i];
            if (st == ZL_OK) {
                memcpy(pr.a, xy1 + i * W1, W1 * 8);
                pr.a_inf = inf1[i];
                st = st2[i];
            }
            if (st == ZL_OK) {
                memcpy(pr.b, xy2 + i * W2, W2 * 8);
                pr.b_inf = inf2[i];
                st = st1[m + i];
            }
            if (st == ZL_OK) {
                memcpy(pr.c, xy1 + (m + i) * W1, W1 * 8);
                pr.c_inf = inf1[m + i];
            }
            status[first + i] = st;
        }
    }
    return ZL_OK;
}
int ZL_DD_SUFFIX(points_host)(zl_group_t group, const uint8_t* in, size_t count, uint64_t* out_xy, uint8_t* out_inf, int32_t* status) {
    if ((group != ZL_G1 && group != ZL_G2) || (count && (!in || !out_xy || !out_inf || !status))) return ZL_EINVAL;
    for (size_t i = 0; i < count; i++)
        status[i] = group == ZL_G1 ? D::decode_g1(in + i * B1, out_xy + i * W1, out_inf + i) : D::decode_g2(in + i * B2, out_xy + i * W2, out_inf + i);
    return ZL_OK;
}
int ZL_DD_SUFFIX(fq2_sqrt)(zl_ctx* ctx, const uint64_t* in, size_t n, uint64_t* out, uint8_t* ok) {
    if (n && (!in || !out || !ok)) return ZL_EINVAL;
    if (n == 0) return ZL_OK;
    if (!ctx) {
        for (size_t i = 0; i < n; i++) fq2_sqrt_one(in + i * NW, out + i * NW, ok + i);
        return ZL_OK;
    }
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    const size_t vb = n * NW * 8;  // bytes of n Fq2 values
    void* d = nullptr;
    const int rc = zl_scratch_get(ctx, ZL_SLOT_TESTHOOK, 2 * up256(vb) + up256(n), &d);
    if (rc) return rc;
    unsigned char* base = static_cast<unsigned char*>(d);
    ZL_HIP(ctx, hipMemcpyAsync(base, in, vb, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_dec_fq2_sqrt, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, reinterpret_cast<const uint64_t*>(base), n,
                       reinterpret_cast<uint64_t*>(base + up256(vb)), base + 2 * up256(vb));
    ZL_HIP(ctx, hipGetLastError());
    ZL_HIP(ctx, hipMemcpyAsync(out, base + up256(vb), vb, hipMemcpyDeviceToHost, ctx->stream));
    ZL_HIP(ctx, hipMemcpyAsync(ok, base + 2 * up256(vb), n, hipMemcpyDeviceToHost, ctx->stream));
    ZL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZL_OK;
}
}  // namespace decode_dev
}  // namespace openzl
