// zl_edwards_dev.h -- what the embedded-curve unit (zl_edwards_dev.hip) offers the other units of the library, beside the C ABI of include/zl_backend_ext.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

// The scalar-multiplication producer of the fused prover (zl_groth16_prove_ed_scalar_muls), under the rules of the Poseidon producers (zl_poseidon_dev.h): HOST
// points (count x point_stride x 8 words, point_stride 0 or 1) and scalars (count x 4 words) -> the assignments of zl_circuit_ed_scalar_mul as rows in DEVICE
// memory (row i at d_rows + i * stride_elems elements, 16-byte aligned); results_out (host, may be null) receives Q = s P of every item, 8 words each.  Inputs
// are staged through ZL_SLOT_EDWARDS in launches of at most ZL_TUNE_ED_CHUNK rows; finished on return; ZL_EINVAL through the flag word for an item the circuit
// refuses.  ctx's device is current; curve and bits are the caller's to check (zl_ed_scalar_mul_assignment_elems).
struct zl_ctx;
int zl_ed_scalar_mul_trace_rows(zl_ctx* ctx, int curve, unsigned bits, const uint64_t* points_xy, size_t point_stride, const uint64_t* scalars, size_t count, void* d_rows,
                                size_t stride_elems, uint64_t* results_out);
// The hybrid-encryption producer of the fused prover (zl_groth16_prove_hybrid_encryptions), under the same rules: HOST generator (one point), ephemeral keys
// (count x 4 words), public keys (count x pk_stride x 8 words, pk_stride 0 or 1), headers (count x header_len) and plaintexts (count x blocks x (width - 1)) ->
// the assignments of zl_circuit_hybrid_encrypt as rows in DEVICE memory; epks_out / tags_out / ciphertexts_out (host, each may be null) receive epk, tag and
// ciphertext of every item.  Two launches a chunk on ctx's stream -- the ladders, one lane per (row, ladder), then the cipher keyed from the row's own cells
// (zl_poseidon_duplex_row_launch) -- both through ZL_SLOT_EDWARDS.  Curve, width, bits, the lengths, initial_state and the generator are checked here as
// zl_hybrid_encrypt_assignments does.
int zl_hybrid_encrypt_trace_rows(zl_ctx* ctx, int curve, unsigned width, unsigned bits, const uint64_t* initial_state, const uint64_t* generator_xy, const uint64_t* esk,
                                 const uint64_t* pks_xy, size_t pk_stride, const uint64_t* headers, size_t header_len, const uint64_t* plaintexts, size_t blocks, size_t count,
                                 void* d_rows, size_t stride_elems, uint64_t* epks_out, uint64_t* tags_out, uint64_t* ciphertexts_out);
