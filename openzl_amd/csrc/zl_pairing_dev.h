// zl_pairing_dev.h -- internal interface of the device Miller loops (zl_pairing_dev.hip, compiled once per curve); used by zl_verify.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/zl_backend_ext.h"

namespace openzl {
namespace pairing_dev {
// Pairs p < n: P_p = ps + p * 2 * FQ64 (x || y canonical), Q_p = qs + p * 4 * FQ64 (x.c0 || x.c1 || y.c0 || y.c1 canonical); all-zero = infinity.
// sc (optional): 4 u32 words (128-bit little-endian scalar) per pair; the pair then is (sc_p P_p, Q_p).
// miller_product_*: prod_p f_p (Montgomery Fq12, 12 x N u32 words), chunked over launch sets of ZL_TUNE_PAIR_SET pairs (default MAX_PAIRS), each set in
// ZL_TUNE_PAIR_GROUPS groups (default 32 per CU): G = ceil(m / groups) pairs share a group, ceil(m / G) groups are launched and padded with ones to G of them
// each.  Both knobs are read per call and exist for the tests (tests/test_gpu_pairing_geometry.py): they reach shared groups, padding and several sets at tens
// of pairs.  miller_groups_*: pair p belongs to group p % ngroups; out receives ngroups Miller products (12 x N words each); n must not exceed MAX_PAIRS;
// ngroups >= 1.
// The values are Miller values times factors of proper subfields (zl_pairing_dev.hip header): only their final exponentiation is defined.
int miller_product_bls(zl_ctx* ctx, const uint64_t* ps, const uint64_t* qs, const uint32_t* sc, size_t n, uint32_t* out);
int miller_groups_bls(zl_ctx* ctx, const uint64_t* ps, const uint64_t* qs, const uint32_t* sc, size_t n, size_t ngroups, uint32_t* out);
int miller_product_bn(zl_ctx* ctx, const uint64_t* ps, const uint64_t* qs, const uint32_t* sc, size_t n, uint32_t* out);
int miller_groups_bn(zl_ctx* ctx, const uint64_t* ps, const uint64_t* qs, const uint32_t* sc, size_t n, size_t ngroups, uint32_t* out);
// final_exp_*: out[i] = in[i]^((q^12 - 1)/r) on the device (k_pd_fexp), Montgomery Fq12 values in host buffers (12 x N words each); singular (optional, count
// bytes): 1 for a zero input, whose result is zero -- what Engine::final_exp leaves and reports for it.  The unique GT value of the host, bit for bit.
// pairing_groups_*: miller_groups_* followed by the final exponentiation of every group, the Miller values staying on the device in between.
// Both run ZL_TUNE_FEXP_CHUNK values per launch (default FEXP_CHUNK).
int final_exp_bls(zl_ctx* ctx, const uint32_t* in, size_t count, uint32_t* out, uint8_t* singular);
int final_exp_bn(zl_ctx* ctx, const uint32_t* in, size_t count, uint32_t* out, uint8_t* singular);
int pairing_groups_bls(zl_ctx* ctx, const uint64_t* ps, const uint64_t* qs, const uint32_t* sc, size_t n, size_t ngroups, uint32_t* out, uint8_t* singular);
int pairing_groups_bn(zl_ctx* ctx, const uint64_t* ps, const uint64_t* qs, const uint32_t* sc, size_t n, size_t ngroups, uint32_t* out, uint8_t* singular);
constexpr size_t FEXP_CHUNK = (size_t)1 << 14;  // values per k_pd_fexp launch: their window powers take 15 x 12 Fq each, 141 MB of HBM for 2^14 BLS12-381 values
constexpr size_t MAX_PAIRS = (size_t)1 << 16;  // pairs per launch set: line stream of 2^16 BLS12-381 pairs = 1.3 GB of HBM
// pairs per launch set for a value of ZL_TUNE_PAIR_SET: clamped to [1, MAX_PAIRS]
inline size_t pair_set(int tune) { return tune < 1 ? 1 : ((size_t)tune < MAX_PAIRS ? (size_t)tune : MAX_PAIRS); }
}  // namespace pairing_dev
}  // namespace openzl
