// zl_decode_dev.h -- internal interface of the device point / proof decoders (zl_decode_dev.hip, compiled once per curve); used by zl_host.hip (the batch decoders; zl_verify.hip's bytes-in
// verifier calls them through zl_groth16_proofs_from_bytes_batch) and zl_testhooks.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/zl_backend_ext.h"

namespace openzl {
namespace decode_dev {
// count compressed points of one group (48 / 96 bytes each for BLS12-381, 32 / 64 for BN254, packed) -> out_xy (count x 2 / 4 Fq of canonical u64 words),
// out_inf (count bytes), status (count codes): per record what zl_point_from_bytes gives.  ZL_OK when the batch ran; count == 0 does nothing.
int points_bls(zl_ctx* ctx, zl_group_t group, const uint8_t* in, size_t count, uint64_t* out_xy, uint8_t* out_inf, int32_t* status);
int points_bn(zl_ctx* ctx, zl_group_t group, const uint8_t* in, size_t count, uint64_t* out_xy, uint8_t* out_inf, int32_t* status);
// count proofs A || B || C -> structs and statuses: per record what zl_groth16_proof_from_bytes gives (one G2 launch over the B's, one G1 launch over the A's and C's)
int proofs_bls(zl_ctx* ctx, const uint8_t* in, size_t count, zl_g16_proof* proofs, int32_t* status);
int proofs_bn(zl_ctx* ctx, const uint8_t* in, size_t count, zl_g16_proof* proofs, int32_t* status);
// test hook: fq2_sqrt of n canonical Fq2 values (c0 || c1 words) on the device (ctx) or the host (null ctx); out = the root (zero when there is none), ok = 0 / 1
int fq2_sqrt_bls(zl_ctx* ctx, const uint64_t* in, size_t n, uint64_t* out, uint8_t* ok);
int fq2_sqrt_bn(zl_ctx* ctx, const uint64_t* in, size_t n, uint64_t* out, uint8_t* ok);
// test hook: the decoders of zl_decode.h on the host
int points_host_bls(zl_group_t group, const uint8_t* in, size_t count, uint64_t* out_xy, uint8_t* out_inf, int32_t* status);
int points_host_bn(zl_group_t group, const uint8_t* in, size_t count, uint64_t* out_xy, uint8_t* out_inf, int32_t* status);
constexpr size_t MAX_RECORDS = (size_t)1 << 18;  // records per launch set (longer batches are chunked): bounds the two scratch slots (BLS12-381 proofs: 48 MB in, 100 MB out)
}  // namespace decode_dev
}  // namespace openzl
