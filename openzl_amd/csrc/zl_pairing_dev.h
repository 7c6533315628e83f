// zl_pairing_dev.h -- internal interface of the device Miller loops (zl_pairing_dev.hip, compiled once per curve); used by zl_host.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/zl_backend_ext.h"

namespace openzl {
namespace pairing_dev {
// Pairs p < n: P_p = ps + p * 2 * FQ64 (x || y canonical), Q_p = qs + p * 4 * FQ64 (x.c0 || x.c1 || y.c0 || y.c1 canonical); all-zero = infinity.
// sc (optional): 4 u32 words (128-bit little-endian scalar) per pair; the pair then is (sc_p P_p, Q_p).
// miller_product_*: prod_p f_p (Montgomery Fq12, 12 x N u32 words), chunked over launches.  miller_groups_*: pair p belongs to group p % ngroups;
// out receives ngroups Miller products (12 x N words each); n must not exceed max_pairs(); ngroups >= 1.
// The values are Miller values times factors of proper subfields (zl_pairing_dev.hip header): only their final exponentiation is defined.
int miller_product_bls(zl_ctx* ctx, const uint64_t* ps, const uint64_t* qs, const uint32_t* sc, size_t n, uint32_t* out);
int miller_groups_bls(zl_ctx* ctx, const uint64_t* ps, const uint64_t* qs, const uint32_t* sc, size_t n, size_t ngroups, uint32_t* out);
int miller_product_bn(zl_ctx* ctx, const uint64_t* ps, const uint64_t* qs, const uint32_t* sc, size_t n, uint32_t* out);
int miller_groups_bn(zl_ctx* ctx, const uint64_t* ps, const uint64_t* qs, const uint32_t* sc, size_t n, size_t ngroups, uint32_t* out);
constexpr size_t MAX_PAIRS = (size_t)1 << 16;  // pairs per launch set: line stream of 2^16 BLS12-381 pairs = 1.3 GB of HBM
}  // namespace pairing_dev
}  // namespace openzl
