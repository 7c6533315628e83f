/* zl_backend_ext.h -- the rest of libzl_backend.so's C ABI: everything beyond the boundary the reference's plugin binds (include/zl_backend.h).
 *
 * Split off in round 6: zl_backend.h holds the drop-in boundary -- the symbols a binding of
 * /root/reference/plugins/arkworks/src/groth16.rs needs: context, bases, zl_msm, zl_ntt, zl_groth16_prove*, the key / proof codecs, verify.  This header
 * holds what the backend offers on top: device-resident and pipelined MSM entry points, partial sums for sharding, the multi-GPU contexts
 * (zl_mctx, zl_msm_sharded, zl_ntt_sharded, zl_groth16_prove_sharded), prover lanes, the C hooks of the C++ host mirror (circuits, compile, prove_circuit),
 * the host pairing, point codecs and timing.  Same conventions, same library. */
#ifndef ZL_BACKEND_EXT_H
#define ZL_BACKEND_EXT_H
#include "zl_backend.h"
#ifdef __cplusplus
extern "C" {
#endif
/* run all work of this ctx on the caller's HIP stream (e.g. torch's current stream); NULL = the ctx's own */
int zl_ctx_set_stream(zl_ctx* ctx, void* hip_stream);
int zl_ctx_sync(zl_ctx* ctx);
/* Pippenger window width c (bits); 0 = choose from n.  Results do not depend on it. */
int zl_ctx_set_msm_window(zl_ctx* ctx, int c);
/* library / device description: writes a NUL-terminated string, returns its length */
int zl_describe(zl_ctx* ctx, char* buf, size_t buflen);
/* bases[i] = k[i] * generator, computed on the device (k: n x 4 u64 canonical, host memory).  Input generator
 * for tests and benches: gives MSM inputs with known discrete logs. */
int zl_bases_generate(zl_ctx* ctx, zl_curve_t curve, zl_group_t group, const uint64_t* k, size_t n, uint64_t* handle_out);
/* copy bases back as canonical affine x||y (tests) */
int zl_bases_download(zl_ctx* ctx, uint64_t handle, size_t first, size_t count, uint64_t* out_xy);
/* multi-GPU building block: the un-normalised partial sum of this shard (opaque, ZL_PARTIAL_WORDS u64s), to
 * be all-gathered (RCCL/ncclUint64) and folded with zl_partials_sum on any rank. */
#define ZL_PARTIAL_WORDS 64
int zl_msm_partial_dev(zl_ctx* ctx, uint64_t bases, size_t first, const void* d_scalars, size_t n, uint64_t* out_partial);
/* `count` MSMs over the same bases range (e.g. the several scalar vectors of one proof, or a stream of proofs against one proving key):
 * d_scalars[i] points to n x 4 u64 canonical scalars in HBM; out_partials receives count x ZL_PARTIAL_WORDS words.  The calls are
 * pipelined on three streams -- the sort of MSM i+2, the bucket accumulation of MSM i+1 and the merge / reduction tail of MSM i
 * overlap -- so that in steady state an MSM costs little more than its accumulation kernel; results are identical to `count` separate calls. */
int zl_msm_batch_partial_dev(zl_ctx* ctx, uint64_t bases, size_t first, const void* const* d_scalars, size_t n, size_t count, uint64_t* out_partials);
/* `count` MSMs over ONE base range in one device pass: vector j = n canonical scalars at d_scalars + j * stride_scalars * 32 bytes
 * (stride_scalars >= n).  out_xy + j * (2 or 4 Fq of canonical words), out_inf[j] (may be NULL): exactly what zl_msm_dev returns for vector j.
 * The batch is the parallel dimension (one wave per vector, 6-bit window and slice of 2048 points; openzl_amd/csrc/zl_msm_multi.hip): measured against
 * zl_msm_batch_partial_dev it is the faster one for many short vectors -- n <= 2^12 with a thousand vectors on every group, G1 from 64 vectors on -- and
 * the slower one at 2^15 points (profiles/prove_batch_bench.log).  A count whose partial sums exceed the scratch budget runs in chunks
 * (ZL_TUNE_MSM_MULTI_CHUNK overrides the chunk).  count == 0 or n == 0: ZL_OK, for n == 0 every result is infinity.  A scalar with bits at or
 * above the scalar field's width: ZL_EINVAL, as from zl_msm_dev. */
int zl_msm_multi_dev(zl_ctx* ctx, uint64_t bases, size_t first, const void* d_scalars, size_t n, size_t stride_scalars, size_t count, uint64_t* out_xy,
                     uint8_t* out_inf);
/* `count` proofs over one key and one resident circuit: assignment j = (n_instance + n_witness) x 4 u64 at assignments + j * that many words (host memory;
 * flags: 0 or ZL_MONT as zl_groth16_prove_resident), blinding scalars r[j], s[j] at r + 4 j, s + 4 j.  proofs[j] equals what
 * zl_groth16_prove_resident returns for (assignment j, r[j], s[j]), byte for byte.  Domains up to 2^ZL_TUNE_G16_BATCH_LOG_N with at least
 * ZL_TUNE_G16_BATCH_MIN proofs keep the whole batch on the device (witness map with a batch dimension, A, B and C as three zl_msm_multi passes over
 * extended queries cached with the key, no point arithmetic on the host); everything else loops the resident prover.  The first failing proof's
 * error is returned.  zl_groth16_last_h after a device batch returns ZL_EINVAL.
 * r, s: canonical, as for zl_groth16_prove.  One r[j] or s[j] at or above the scalar field's modulus refuses the whole call with ZL_EINVAL before any device
 * work, on either path and whatever its index; no proof is written.  The same holds for every batched prover below (_batch_dev, _poseidon_chains, _merkle_*,
 * _forest_members, _poseidon_hashes, _merkle_leaf_*, _poseidon_encryptions, _ed_scalar_muls) and for zl_groth16_prove_sharded. */
int zl_groth16_prove_batch(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, const uint64_t* assignments, unsigned flags, const uint64_t* r,
                           const uint64_t* s, size_t count, zl_g16_proof* proofs);
/* The same with the assignments in DEVICE memory (count x (n_instance + n_witness) elements, densely): on the device path every chunk is one device-to-device
 * copy into the batch's block; where the dispatch bounds send the batch to the loop over the resident prover -- it reads its assignment from host memory -- the
 * assignments come back through host staging of at most 64 MiB at a time.  r, s and proofs are host memory.  Same proofs, same error codes. */
int zl_groth16_prove_batch_dev(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, const void* d_assignments, unsigned flags, const uint64_t* r,
                               const uint64_t* s, size_t count, zl_g16_proof* proofs);
/* Poseidon-chain inputs in, proofs out: proofs[j] = what zl_groth16_prove_resident returns for the assignment of zl_circuit_poseidon_chain(curve, k, x0[j], x1[j])
 * (zl_poseidon_chain_assignments below) with r[j], s[j], byte for byte; x0, x1, r, s: count x 4 u64 in host memory; public_out (may be NULL) receives h_k per
 * proof, the public input.  On the device path of zl_groth16_prove_batch the trace kernel of zl_poseidon_dev.hip writes every chunk's assignments straight into
 * the chunk's block of the batch (inputs staged in chunks of at most ZL_TUNE_POSEIDON_CHUNK chains): no assignment crosses the bus or exists in host memory.
 * Off it, assignments are produced zl_poseidon_chain_assignments-wise, at most 64 MiB at a time, for the loop over the resident prover.  The resident circuit
 * must have the SHAPE of a k-link chain (n_instance == 2, n_witness == 2 + 234 k, n_constraints == 234 k + 1), else ZL_EINVAL; what its matrices hold cannot be
 * checked -- as with a witness-only compiler, a different circuit of that shape yields proofs that do not verify.  k == 0, an input >= r, or -- off the
 * device path only -- a k above zl_poseidon_chain_assignments' 35 848: ZL_EINVAL; the
 * other error codes and their order are those of zl_groth16_prove_batch. */
int zl_groth16_prove_poseidon_chains(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, uint32_t k, const uint64_t* x0, const uint64_t* x1, const uint64_t* r,
                                     const uint64_t* s, size_t count, zl_g16_proof* proofs, uint64_t* public_out);
/* Merkle memberships in, proofs out: zl_groth16_prove_poseidon_chains with another producer.  proofs[j] = what zl_groth16_prove_resident returns for the
 * assignment of zl_circuit_poseidon_merkle (zl_poseidon_merkle_assignments below) with r[j], s[j], byte for byte.
 *   _paths:   leaves (count x 4 u64), indices (count u64) and paths (count x depth x 4 u64) in HOST memory; roots_out (may be NULL) receives the root of every
 *             fold, the public input of proof j.  An index >= 2^depth is ZL_EINVAL before any work.
 *   _members: a node array in DEVICE memory (zl_poseidon_merkle_build_dev: n leaves, `depth` levels) and HOST indices: proof j shows that leaf indices[j] is in
 *             the tree.  Nothing but the indices and the blinding scalars goes up; root_out (may be NULL) receives the one root, every proof's public input.
 *             n > 2^depth or an index >= n is ZL_EINVAL before any work.
 * On the device path the trace kernel writes every chunk's rows straight into the chunk's block; off it, rows are produced at most 64 MiB at a time for the
 * loop over the resident prover (_members: written by the device and downloaded).  The dispatch bounds are zl_groth16_prove_batch's and are not moved: depth <= 8
 * has a domain of at most 2^11, so from 64 proofs on it stays on the device by default; deeper paths loop the resident prover -- there the gain is that
 * synthesis and the assignments' way over the bus are gone, not the batched MSMs.  The resident circuit must have the SHAPE of a depth-d membership circuit
 * (n_instance, n_witness, n_constraints) == (2, 1 + 238 d, 237 d + 1), else ZL_EINVAL; what its matrices hold cannot be checked.  No chain shape
 * (2, 2 + 234 k, 234 k + 1) equals a membership shape for integers k, d >= 1: n_witness - n_constraints is 1 for a chain and d for a membership, so d = 1, and
 * then 234 k = 237 has no solution -- keys of a chain are refused here and keys of a membership by zl_groth16_prove_poseidon_chains.  A depth outside 1..40 or
 * an input >= r: ZL_EINVAL; the other error codes and their order are those of zl_groth16_prove_batch. */
int zl_groth16_prove_merkle_paths(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, unsigned depth, const uint64_t* leaves, const uint64_t* indices,
                                  const uint64_t* paths, const uint64_t* r, const uint64_t* s, size_t count, zl_g16_proof* proofs, uint64_t* roots_out);
int zl_groth16_prove_merkle_members(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, const void* d_nodes, size_t n, unsigned depth, const uint64_t* indices,
                                    const uint64_t* r, const uint64_t* s, size_t count, zl_g16_proof* proofs, uint64_t* root_out);
/* The same out of a Merkle forest in device memory (zl_merkle_forest_* below): proof j shows that leaf indices[j] of tree tree_of[j] is in that tree, and is
 * byte for byte what zl_groth16_prove_merkle_members returns on zl_merkle_forest_tree_nodes(f, tree_of[j]) with n = the forest's capacity and (r[j], s[j]).
 * tree_of (count u32) and indices are HOST memory; roots_out (count x 4 u64, may be NULL) receives the root per proof -- the trees differ.  ctx is the forest's
 * ctx or another lane of its device; the depth is the forest's.  Shape check, dispatch bounds and error order are zl_groth16_prove_merkle_members'; a NULL or
 * host-mirror forest, a forest over another curve than the key's, a tree id >= trees or an index >= that tree's length: ZL_EINVAL before any work. */
typedef struct zl_merkle_forest zl_merkle_forest;
int zl_groth16_prove_forest_members(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, const zl_merkle_forest* f, const uint32_t* tree_of, const uint64_t* indices,
                                    const uint64_t* r, const uint64_t* s, size_t count, zl_g16_proof* proofs, uint64_t* roots_out);
/* The same three producers for the arity-general circuits (zl_circuit_poseidon_hash / _merkle_leaf below): proofs[j] = what zl_groth16_prove_resident returns
 * for row j of zl_poseidon_hash_assignments resp. zl_poseidon_merkle_leaf_assignments with r[j], s[j], byte for byte.
 *   _poseidon_hashes:      in (count x arity x 4 u64, HOST); public_out (may be NULL) receives the digest per proof.
 *   _merkle_leaf_paths:    preimages (count x arity), indices (count u64) and paths (count x depth) in HOST memory; roots_out (may be NULL) the root per proof.
 *   _merkle_leaf_members:  a node array (zl_poseidon_merkle_build_dev: n leaves, `depth` levels) and the n x arity preimages of its leaves in DEVICE memory, HOST
 *                          indices; root_out (may be NULL) receives the one root.  A preimage that does not hash to its leaf is ZL_EINVAL, as in
 *                          zl_poseidon_merkle_leaf_member_assignments_dev.
 * Each call checks that the resident circuit has the SHAPE of the stated (arity, depth) -- (2, a + 3 S(a), 3 S(a) + 1) resp. (2, a + 3 S(a) + 238 d,
 * 3 S(a) + 237 d + 1) -- else ZL_EINVAL; the shapes of the four families are told apart in the note at zl_circuit_poseidon_hash.  Error order and dispatch
 * bounds are zl_groth16_prove_batch's and are not moved (a hash circuit has a domain of 2^8 or 2^9, a leaf membership of depth <= 7 at most 2^11); off the
 * device path the rows come through host staging as for the membership producers.  arity outside 2..5, depth outside 1..40, an index >= 2^depth (>= n), n >
 * 2^depth or an input >= r: ZL_EINVAL. */
int zl_groth16_prove_poseidon_hashes(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, unsigned arity, const uint64_t* in, const uint64_t* r, const uint64_t* s,
                                     size_t count, zl_g16_proof* proofs, uint64_t* public_out);
int zl_groth16_prove_merkle_leaf_paths(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, unsigned arity, unsigned depth, const uint64_t* preimages,
                                       const uint64_t* indices, const uint64_t* paths, const uint64_t* r, const uint64_t* s, size_t count, zl_g16_proof* proofs,
                                       uint64_t* roots_out);
int zl_groth16_prove_merkle_leaf_members(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, unsigned arity, const void* d_nodes, const void* d_preimages, size_t n,
                                         unsigned depth, const uint64_t* indices, const uint64_t* r, const uint64_t* s, size_t count, zl_g16_proof* proofs,
                                         uint64_t* root_out);
int zl_partials_sum(zl_curve_t curve, zl_group_t group, const uint64_t* partials, size_t count, uint64_t* out_xy, uint8_t* out_inf);
/* wrap a canonical affine point (all-zero = infinity) as a partial, e.g. to fold an extra term into zl_partials_sum */
int zl_partial_from_affine(zl_curve_t curve, zl_group_t group, const uint64_t* xy, uint64_t* out_partial);
/* Multi-GPU transform (ark-poly has no distributed form -- same function as zl_ntt on the 2^log_n
 * domain, split over G = 2^log_g ranks, M = N/G elements each, B = M/G, with ONE all-to-all between the two local steps):
 *   block-column layout: rank g holds x[j1*M + g*B + c] at local [j1*B + c]  (j1 < G, c < B)
 *   cyclic layout:       rank k holds X[k + G*k2]       at local [k2]        (k2 < M)
 *   forward: zl_ntt_cross_dev (block-column data) -> all-to-all of G chunks of B elements -> zl_ntt_dev(log_n - log_g)
 *            leaves the evaluations in cyclic layout;
 *   inverse: zl_ntt_dev(log_n - log_g, ZL_INVERSE) on cyclic data -> all-to-all -> zl_ntt_cross_dev(ZL_INVERSE)
 *            leaves the coefficients in block-column layout.
 * zl_ntt_cross_dev does the G-point transform across the G local rows of each column, the w_N^(j2 k1) twiddle, and the
 * ZL_COSET scaling of the whole 2^log_n domain; the local M-point leg is always called WITHOUT ZL_COSET.  Elements are
 * Montgomery between the legs (ZL_MONT_IN / ZL_MONT_OUT pick the outer representation).  1 <= log_g <= 4, 2*log_g <= log_n.
 * openzl_amd/sharded.py drives the three steps over torch.distributed (RCCL all_to_all_single). */
int zl_ntt_cross_dev(zl_ctx* ctx, zl_curve_t curve, void* d_data, unsigned log_n, unsigned log_g, unsigned rank, unsigned flags);
/* `count` transforms of the same size and flags in one launch per pass: vector v starts at d_data + v * stride_elems elements (stride_elems >= 2^log_n).  What the
 * Groth16 witness map does with its a, b, c vectors (groth16.rs:445-457 -> ark-groth16's witness map: three iffts, three coset ffts): below ~2^16 elements a transform
 * is a chain of latency-bound passes, and three of them cost what one does.  Results are those of `count` zl_ntt_dev calls. */
int zl_ntt_batch_dev(zl_ctx* ctx, zl_curve_t curve, void* d_data, unsigned log_n, unsigned flags, unsigned count, size_t stride_elems);

/* ---- multi-GPU in one process: G devices, one zl_ctx each, RCCL (ncclCommInitAll) between them ------------------
 * Upload / generate / precompute every rank's shard of the bases on ITS ctx (zl_mctx_ctx(m, rank)) with the single-device calls above.
 * device_ids may repeat (several "virtual ranks" on one GPU, for testing on a 1-GPU box): RCCL refuses duplicate devices, so the
 * exchanges then run as device-to-device copies with the same data movement pattern; zl_mctx_uses_rccl tells which.  1 <= n_devices <= 16.
 * Callers that run one process per GPU instead use zl_msm_partial_dev + their own all-gather + zl_partials_sum (openzl_amd/sharded.py). */
typedef struct zl_mctx zl_mctx;
int zl_ctx_create_multi(zl_mctx** out, const int* device_ids, int n_devices);
void zl_mctx_destroy(zl_mctx* m);
int zl_mctx_size(const zl_mctx* m);
zl_ctx* zl_mctx_ctx(zl_mctx* m, int rank);
int zl_mctx_uses_rccl(const zl_mctx* m);
int zl_mctx_last_rccl_error(const zl_mctx* m);
/* Sharded MSM (config 4: 2^26 as 8 x 2^23): rank g holds bases handle bases[g] on its ctx and n[g] canonical scalars in ITS device memory
 * (d_scalars[g]); first may be NULL.  Every device runs the complete local Pippenger concurrently, the G un-normalised partial sums
 * (ZL_PARTIAL_WORDS u64 each) are all-gathered (ncclAllGather as ncclUint64; EC addition is no RCCL reduction op, so gather-then-add
 * IS the reduce) and folded: out_xy = canonical affine sum over all shards. */
int zl_msm_sharded(zl_mctx* m, const uint64_t* bases, const size_t* first, const void* const* d_scalars, const size_t* n, uint64_t* out_xy,
                   uint8_t* out_inf);
/* ONE 2^log_n transform over G = 2^log_g ranks (layouts and legs: zl_ntt_cross_dev below): d_data[g] = rank g's M = 2^(log_n - log_g)
 * elements in its device memory, in place.  forward: block-column coefficients in, cyclic evaluations out; ZL_INVERSE: the reverse.
 * One all-to-all (grouped ncclSend / ncclRecv of G chunks of M/G elements per rank) between the two local legs.  flags: ZL_MONT,
 * ZL_COSET, ZL_INVERSE. */
int zl_ntt_sharded(zl_mctx* m, zl_curve_t curve, void* const* d_data, unsigned log_n, unsigned flags);
/* ONE proof over the G devices of an mctx: the five MSMs of create_proof_with_assignment shard by point range like any MSM.  Rank g holds, on
 * zl_mctx_ctx(m, g), bases handles with ITS contiguous slice of every query -- a / b_g1 / b_g2 over the variables [var_first, var_first + var_count) (variable 0
 * is the constant ONE), l over the witnesses [wit_first, ...), h over the domain indices [h_first, ...) of the N - 1 quotient coefficients -- uploaded with the
 * single-device calls; the slices of consecutive ranks must tile the three ranges in rank order (a rank may hold empty slices: count 0, handle ignored).
 * Rank 0 also holds the constraint matrices (r1cs_handle_rank0 from zl_r1cs_upload on zl_mctx_ctx(m, 0)) and runs the witness map; the other ranks receive
 * their slices of z and h by device-to-device copy, every rank runs its five partial MSMs, the host folds the partials over the ranks and assembles the proof.
 * pk: only curve and the five single points are read.  The proof equals zl_groth16_prove_resident's for the same (r, s), byte for byte. */
typedef struct zl_g16_shard {
    uint64_t a_query, b_g1_query, h_query, l_query; /* ZL_G1 handles on this rank's ctx: var_count, var_count, h_count, wit_count points */
    uint64_t b_g2_query;                            /* ZL_G2 handle: var_count points */
    size_t var_first, var_count, wit_first, wit_count, h_first, h_count;
} zl_g16_shard;
int zl_groth16_prove_sharded(zl_mctx* m, const zl_g16_pk* pk, const zl_g16_shard* shards, uint64_t r1cs_handle_rank0, const uint64_t* assignment,
                             unsigned flags, const uint64_t* r, const uint64_t* s, zl_g16_proof* out);
/* the quotient polynomial h of the last successful zl_groth16_prove* call on this ctx (N x 4 u64 canonical), for tests;
 * ZL_EINVAL when there is none (it lives in the Groth16 scratch block of the ctx and is invalidated when the next proof starts) */
int zl_groth16_last_h(zl_ctx* ctx, uint64_t* out, size_t n);

/* ---- host mirror of the plugin interface (C hooks over the C++ classes of openzl_amd/csrc/zl_host.h) ------------
 * openzl::R1CS<F> / poseidon gadget / Groth16<E>::{compile, prove} restated in C++ (the reference is Rust; no Rust
 * toolchain here).  These hooks let a C / ctypes caller drive them; a C++ caller uses the classes directly.  Circuits, keys, proving and the wire
 * formats are implemented in csrc/zl_host.hip; Groth16<E>::verify, zl_pairing*, zl_groth16_verify* in csrc/zl_verify.hip. */
typedef struct zl_circuit zl_circuit;   /* an R1CS<F> compiler in proof mode holding the config-5 circuit */
/* k chained Poseidon arity-2 hashes over the curve's Fr: h_1 = H(x0,x1), h_{j+1} = H(h_j,x1), public input h_k */
int zl_circuit_poseidon_chain(zl_curve_t curve, uint32_t k, const uint64_t* x0, const uint64_t* x1, zl_circuit** out);
/* The same circuit run by a WITNESS-ONLY compiler (ark-relations' SynthesisMode::Prove { construct_matrices: false }): variables with their values, no linear
 * combinations, no constraint rows -- ~10x faster to synthesise.  zl_groth16_prove_circuit takes it for keys that already hold the circuit's matrices (compiled
 * for it, or bound by an earlier proof with a full circuit); zl_circuit_export then yields an empty CSR and the assignment, zl_circuit_is_satisfied checks only
 * the enforced equalities. */
int zl_circuit_poseidon_chain_witness(zl_curve_t curve, uint32_t k, const uint64_t* x0, const uint64_t* x1, zl_circuit** out);
void zl_circuit_free(zl_circuit* c);
/* CSR view + assignment (pointers stay valid until zl_circuit_free) */
int zl_circuit_export(const zl_circuit* c, zl_r1cs* view, const uint64_t** assignment);
int zl_circuit_is_satisfied(const zl_circuit* c); /* 1 / 0 */
/* native Poseidon permutation, width 3 (tutorial schedule): state = 3 x 4 u64 canonical, in place */
int zl_poseidon_permute(zl_curve_t curve, uint64_t* state);
/* ---- batched Poseidon (openzl_amd/csrc/zl_poseidon_dev.hip): the same width-3 permutation (8 full + 55 partial rounds, x^5, tutorial schedule) for many
 * states at once, one device lane per permutation.  H(x, y) = element 0 of permute([3, x, y]) -- 3 is the arity-2 domain tag of the circuit's hash
 * (openzl-crypto/src/poseidon/hash.rs:93-135) -- so H is the hash zl_circuit_poseidon_chain proves.  Every field element is 4 u64 canonical (< r).
 * Common rules: count == 0 is ZL_OK and nothing is written; an input element >= r is ZL_EINVAL (the kernels raise a flag word; the outputs are then
 * unspecified); null pointers, an unknown curve, a depth outside 1..40 or n > 2^depth are ZL_EINVAL.  On the entry points that take HOST pointers ctx may
 * be NULL: the call then runs the host mirror's permutation over the library's host thread pool and opens no device; with a ctx, batches below
 * ZL_TUNE_POSEIDON_DEV_MIN items take that host path too.  Host batches are staged through one scratch slot of the ctx under a byte budget, in chunks of at
 * most ZL_TUNE_POSEIDON_CHUNK permutations (also the permutations of one launch).  Every call has FINISHED when it returns: it reads the flag word back on
 * the ctx's stream (zl_ctx_set_stream is honoured) and waits for it. */
int zl_poseidon_permute_batch(zl_ctx* ctx, zl_curve_t curve, uint64_t* states, size_t count); /* count x 3 elements, in place: state i as zl_poseidon_permute */
int zl_poseidon_hash2_batch(zl_ctx* ctx, zl_curve_t curve, const uint64_t* xy, size_t count, uint64_t* out); /* out[i] = H(xy[2i], xy[2i+1]) */
/* the same on DEVICE pointers (count x 2 elements in, count elements out; they may not overlap): never the host path, ctx == NULL is ZL_EINVAL */
int zl_poseidon_hash2_batch_dev(zl_ctx* ctx, zl_curve_t curve, const void* d_xy, size_t count, void* d_out);
/* ---- every arity the reference specifies (plugins/arkworks/src/poseidon/mod.rs:300-322): arity 2, 3, 4, 5 = width 3, 4, 5, 6 with 8 full and 55, 55, 56, 56
 * partial rounds; the hash of `arity` inputs is element 0 of permute([2^arity - 1, x_1 .. x_arity]) (openzl-crypto/src/poseidon/hash.rs:64-135).  The round keys
 * come from the reference's LFSR seeded with (field bits, width, full, partial) and the MDS entry [i][j] is 1 / (i + width + j), as at width 3.  The reference
 * states the table for BN254; BLS12-381 Fr takes the same rows here.  The common rules above hold unchanged; at width 3 / arity 2 every call below returns byte
 * for byte what its width-3 counterpart returns.  In circuit, the chain and the inner hash of the Merkle levels stay arity 2; zl_circuit_poseidon_hash and
 * zl_circuit_poseidon_merkle_leaf below prove one hash, and a membership whose leaf is hashed from a preimage, at every arity of the table. */
/* width, rounds and tag of an arity (a NULL output is skipped); ZL_EINVAL outside 2..5 */
int zl_poseidon_spec(unsigned arity, unsigned* width, unsigned* full_rounds, unsigned* partial_rounds, uint64_t* tag);
/* host, one state of `width` elements in place (width 3..6; elements are taken as zl_poseidon_permute takes them); width 3 == zl_poseidon_permute */
int zl_poseidon_permute_w(zl_curve_t curve, unsigned width, uint64_t* state);
/* the generated constants, canonical: width * (full + partial) keys [width * round + lane], width * width MDS entries row-major; either may be NULL */
int zl_poseidon_constants(zl_curve_t curve, unsigned width, uint64_t* keys, uint64_t* mds);
/* batched, host pointers: the common rules of zl_poseidon_permute_batch (NULL ctx / below ZL_TUNE_POSEIDON_DEV_MIN -> host pool; staged in chunks of
 * ZL_TUNE_POSEIDON_CHUNK items of `width` resp. `arity` + 1 elements under the byte budget; finished on return).  states: count x width elements, in place;
 * in: count x arity elements, out: count digests */
int zl_poseidon_permute_batch_w(zl_ctx* ctx, zl_curve_t curve, unsigned width, uint64_t* states, size_t count);
int zl_poseidon_hash_batch(zl_ctx* ctx, zl_curve_t curve, unsigned arity, const uint64_t* in, size_t count, uint64_t* out);
/* device pointers, never the host path (ctx == NULL is ZL_EINVAL); in and out may not overlap */
int zl_poseidon_hash_batch_dev(zl_ctx* ctx, zl_curve_t curve, unsigned arity, const void* d_in, size_t count, void* d_out);
/* ---- the duplex-sponge authenticated cipher over the same permutation: the reference's FixedDuplexer<N, Spec<F, ARITY>> (openzl-crypto/src/permutation/duplex.rs,
 * sponge.rs; poseidon/encryption.rs), width W = ARITY + 1 in 3..6, rate W - 1: lanes 1 .. W - 1 of the state, lane 0 is never written.  Per message:
 *   setup blocks  padded_chunks_with(key, rate, 0) followed by padded_chunks_with(header, rate, 0) (openzl-util/src/vec.rs:60-77), which ALWAYS ends in one more,
 *                 zero-padded chunk: a key of exactly `rate` elements gives its block and an all-zero block, an empty header one all-zero block;
 *                 SB = key_len / rate + 1 + header_len / rate + 1 >= 2.  Absorbing block b: state[1 + i] += b[i], then permute;
 *   encrypt j     state[1 + i] += p[j][i]; c[j][i] = state[1 + i], read before the permutation; then permute;
 *   decrypt j     p[j][i] = c[j][i] - state[1 + i]; state[1 + i] = c[j][i]; then permute;
 *   tag           state[1] after the last permutation (Tag::read).
 * SB + blocks dependent permutations per message (zl_poseidon_duplex_permutations; 0 for a parameter out of range), all inside one launch, one device lane per
 * message (k_pos_duplex).  initial_state: W elements shared by the batch (FixedEncryption::initial_state), host memory in every form, NULL = the zero state.
 * Dense layouts: item i's key at element i * key_len, its header at i * header_len, its text at i * blocks * rate, its tag at i; keys may be NULL when key_len is 0,
 * headers when header_len is 0.  A fixed-length message: the caller pads.  The output text may be exactly the input text pointer (in place); any other overlap is
 * the caller's error.  Decryption writes the plaintext of EVERY item and reports per item whether the computed tag equals the given one (ok_each[i] = 1 / 0, the
 * reference's (bool, plaintext)): a tag mismatch is not an error, the call returns ZL_OK.
 * The common rules of the batched Poseidon entry points hold (count == 0 is ZL_OK and writes nothing; ctx == NULL or a count below ZL_TUNE_POSEIDON_DEV_MIN runs
 * the host mirror, poseidon::duplex_encrypt / duplex_decrypt of csrc/zl_host.h, over the host pool; otherwise staged in chunks of ZL_TUNE_POSEIDON_CHUNK items
 * under the byte budget; finished on return; results are byte-identical on every path).  ZL_EINVAL: width outside 3..6, key_len or header_len above 64, blocks
 * outside 1..1024 (one launch is one dependent chain: the cap keeps it near a second at width 6), a null required pointer, an unknown curve, any element >= r --
 * initial_state is checked on the host before any work, the rest through the flag word.  The _dev forms take DEVICE pointers for keys, headers, texts and tags
 * (never the host path: ctx == NULL is ZL_EINVAL); initial_state and ok_each stay host memory. */
size_t zl_poseidon_duplex_permutations(unsigned width, size_t key_len, size_t header_len, size_t blocks);
int zl_poseidon_duplex_encrypt_batch(zl_ctx* ctx, zl_curve_t curve, unsigned width, const uint64_t* initial_state, const uint64_t* keys, size_t key_len,
                                     const uint64_t* headers, size_t header_len, const uint64_t* plaintexts, size_t blocks, size_t count, uint64_t* ciphertexts,
                                     uint64_t* tags);
int zl_poseidon_duplex_decrypt_batch(zl_ctx* ctx, zl_curve_t curve, unsigned width, const uint64_t* initial_state, const uint64_t* keys, size_t key_len,
                                     const uint64_t* headers, size_t header_len, const uint64_t* ciphertexts, const uint64_t* tags, size_t blocks, size_t count,
                                     uint64_t* plaintexts, uint8_t* ok_each);
int zl_poseidon_duplex_encrypt_batch_dev(zl_ctx* ctx, zl_curve_t curve, unsigned width, const uint64_t* initial_state, const void* d_keys, size_t key_len,
                                         const void* d_headers, size_t header_len, const void* d_plaintexts, size_t blocks, size_t count, void* d_ciphertexts,
                                         void* d_tags);
int zl_poseidon_duplex_decrypt_batch_dev(zl_ctx* ctx, zl_curve_t curve, unsigned width, const uint64_t* initial_state, const void* d_keys, size_t key_len,
                                         const void* d_headers, size_t header_len, const void* d_ciphertexts, const void* d_tags, size_t blocks, size_t count,
                                         void* d_plaintexts, uint8_t* ok_each);
/* The cipher in circuit (host compilers): "the public ciphertext and tag are the encryption, under a secret key and the public header, of a secret plaintext".
 * initial_state (NULL = zero) and the padding are constants; key_len >= 1 (with no key nothing is secret and leading permutations would fold away).
 * Public inputs: the tag, the blocks x rate ciphertext elements (Ciphertext::extend: tag, then message), the header_len header elements.  Witnesses: the key, the
 * plaintext, then the S-box records (x^2, x^4, x^5) of the SB + blocks permutations in execution order, round order, lane order within a round.  Rows: the
 * records', then tag = public tag, then one row a * 1 = c per ciphertext element.  Additions are linear and allocate nothing; constant folding decides which
 * S-boxes exist: in the first permutation lane 0 of round 0 folds and so does every rate lane without a key element, Z = max(0, rate - key_len) of them; every
 * later permutation records all F = 8 W + partial S-boxes.  S = (F - 1 - Z) + (SB + blocks - 1) F, and the shape (n_instance, n_witness, n_constraints) is
 * (2 + blocks rate + header_len, key_len + blocks rate + 3 S, 3 S + 1 + blocks rate).  n_instance >= 4 where every other circuit family has 2: no family's prover
 * takes another's keys.  _witness: the same circuit in the witness-only compiler, assignments equal word for word.  These circuits go through
 * zl_groth16_compile, zl_groth16_prove_circuit and the batched prover as any circuit does.  ZL_EINVAL as above, and for key_len == 0. */
int zl_circuit_poseidon_encrypt(zl_curve_t curve, unsigned width, const uint64_t* initial_state, const uint64_t* key, size_t key_len, const uint64_t* header,
                                size_t header_len, const uint64_t* plaintext, size_t blocks, zl_circuit** out);
int zl_circuit_poseidon_encrypt_witness(zl_curve_t curve, unsigned width, const uint64_t* initial_state, const uint64_t* key, size_t key_len, const uint64_t* header,
                                        size_t header_len, const uint64_t* plaintext, size_t blocks, zl_circuit** out);
/* The complete ASSIGNMENTS of the encryption circuit, one device lane per row (k_pos_duplex_trace: the cipher's SB + blocks dependent permutations of one launch
 * under a recorder), word for word what both compilers export, rate = W - 1:
 *   [0] = 1   [1] = tag   [2 .. 2 + blocks rate) ciphertext   [.. + header_len) header   [.. + key_len) key   [.. + blocks rate) plaintext   then the 3 S records
 * zl_poseidon_encrypt_assignment_elems = n_instance + n_witness = 2 + 2 blocks rate + header_len + key_len + 3 S; 0 for a parameter out of range (width outside
 * 3..6, key_len 0 or above 64, header_len above 64, blocks outside 1..1024) or a count that does not fit 31 bits.  Dense layouts as the cipher's.  The host-pointer
 * form writes count dense rows under the common rules of the batched Poseidon entry points (ctx == NULL or a count below ZL_TUNE_POSEIDON_DEV_MIN: the host
 * mirror over the host pool, byte-identical; staged in chunks of ZL_TUNE_POSEIDON_CHUNK under the 256 MiB budget; finished on return; an element >= r is ZL_EINVAL
 * through the flag word; every row within the limits fits the budget with its inputs, so the chains' refusal of an over-long row has no case here).  The _dev
 * form takes DEVICE pointers and never the host path (ctx == NULL is ZL_EINVAL): row i starts at d_out + i * stride_elems elements, stride_elems >= the row length,
 * elements behind the row are not written, d_out must be 16-byte aligned and must not overlap the inputs.  initial_state is HOST memory in every form, NULL =
 * zero, checked on the host before any work.  ZL_EINVAL: the cipher's errors plus the circuit's -- a parameter out of range as above, a null required pointer
 * (headers may be NULL when header_len is 0), an unknown curve.
 * zl_groth16_prove_poseidon_encryptions: from HOST keys, headers and plaintexts to proofs -- proofs[j] is byte for byte what zl_groth16_prove_resident returns for
 * row j with (r[j], s[j]); tags_out (count x 4 u64) and ciphertexts_out (count x blocks rate x 4 u64), either may be NULL, receive what
 * zl_poseidon_duplex_encrypt_batch computes: the cipher runs ONCE.  On the device path the kernel writes each chunk's rows into the chunk's block; off it the rows
 * come through host staging of at most 64 MiB at a time.  The resident circuit must have the SHAPE (2 + N rate + H, K + N rate + 3 S, 3 S + 1 + N rate) of the
 * stated parameters, else ZL_EINVAL; error order and dispatch bounds are zl_groth16_prove_batch's and are not moved ((K, H, N) = (2, 0, 1) has a domain of 2^10 at
 * every width).  Device-resident inputs: _assignments_dev, then zl_groth16_prove_batch_dev.
 * SHAPES.  n_instance >= 4 tells this family from every other (2) but one: the scalar-multiplication circuits (zl_circuit_ed_scalar_mul) have n_instance = 5,
 * and cannot share a shape with an encryption -- theirs is (5, 14 bits - 10, 14 bits - 8), which would need K = n_witness - (n_constraints - 1) = -1.  Within it the shape fixes K, N rate, H and S: n_witness - (n_constraints - 1) = K, then
 * n_witness = K + N rate + 3 S and n_constraints = 3 S + 1 + N rate give N rate and S, and n_instance = 2 + N rate + H gives H.  At ONE width two tuples of one
 * shape are therefore the same tuple.  Across widths they need N (W - 1) = N' (W' - 1) and S(W, K, H, N) = S(W', K, H, N'); an exhaustive walk over the limits
 * (tests/test_poseidon_encrypt_assignments_cpu.py repeats it) finds exactly ONE such pair: (W, K, H, N) = (5, 15, 15, 5) and (6, 15, 15, 4), both with 20 text
 * elements and S = 1 247.  Those two are different circuits of one shape: the call cannot refuse the keys of one for the parameters of the other, and the proofs
 * do not verify -- as for keys compiled from ANY other circuit of the same shape, in every family.  Every other tuple's keys are refused. */
size_t zl_poseidon_encrypt_assignment_elems(unsigned width, size_t key_len, size_t header_len, size_t blocks);
int zl_poseidon_encrypt_assignments(zl_ctx* ctx, zl_curve_t curve, unsigned width, const uint64_t* initial_state, const uint64_t* keys, size_t key_len,
                                    const uint64_t* headers, size_t header_len, const uint64_t* plaintexts, size_t blocks, size_t count, uint64_t* out);
int zl_poseidon_encrypt_assignments_dev(zl_ctx* ctx, zl_curve_t curve, unsigned width, const uint64_t* initial_state, const void* d_keys, size_t key_len,
                                        const void* d_headers, size_t header_len, const void* d_plaintexts, size_t blocks, size_t count, void* d_out, size_t stride_elems);
int zl_groth16_prove_poseidon_encryptions(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, unsigned width, const uint64_t* initial_state, const uint64_t* keys,
                                          size_t key_len, const uint64_t* headers, size_t header_len, const uint64_t* plaintexts, size_t blocks, const uint64_t* r,
                                          const uint64_t* s, size_t count, zl_g16_proof* proofs, uint64_t* tags_out, uint64_t* ciphertexts_out);
/* out[i] = h_k with h_1 = H(x0[i], x1[i]), h_{j+1} = H(h_j, x1[i]): the public input of zl_circuit_poseidon_chain(curve, k, x0[i], x1[i]); the k dependent
 * hashes of a chain run inside one kernel.  k == 0: ZL_EINVAL, as zl_circuit_poseidon_chain. */
int zl_poseidon_chain_batch(zl_ctx* ctx, zl_curve_t curve, const uint64_t* x0, const uint64_t* x1, uint32_t k, size_t count, uint64_t* out);
/* The complete ASSIGNMENT of zl_circuit_poseidon_chain(curve, k, x0[i], x1[i]) per chain, the witness a prover of the chain needs, computed where the chain is:
 *   [0] = 1   [1] = h_k   [2] = x0   [3] = x1   then for link j = 1..k, in round order, x^2, x^4, x^5 of every S-box except lane 0 of round 0 (its input is
 *   the domain tag plus a round key: a constant the circuit folds) -- 78 S-boxes, 234 elements per link.
 * zl_poseidon_chain_assignment_elems(k) = 4 + 234 k elements per chain (0 for k == 0 or a count that does not fit 31 bits); word for word what the host
 * compilers (full and witness-only) export.  The host-pointer form writes count dense rows and follows the common rules above (ctx == NULL or a count below
 * ZL_TUNE_POSEIDON_DEV_MIN: the host mirror over the host pool); it stages whole rows, so a row with its inputs must fit the 256 MiB staging budget: k above
 * 35 848 is ZL_EINVAL there, on either path.  The _dev form takes device pointers (never the host path; ctx == NULL is ZL_EINVAL) and any k the element
 * count allows: row i starts at d_out + i * stride_elems elements, stride_elems >= the row length, elements behind the row are not written; d_out must be
 * 16-byte aligned and the rows must not overlap d_x0 or d_x1 (the inputs are read again after a row's records are stored). */
size_t zl_poseidon_chain_assignment_elems(uint32_t k);
int zl_poseidon_chain_assignments_dev(zl_ctx* ctx, zl_curve_t curve, const void* d_x0, const void* d_x1, uint32_t k, size_t count, void* d_out, size_t stride_elems);
int zl_poseidon_chain_assignments(zl_ctx* ctx, zl_curve_t curve, const uint64_t* x0, const uint64_t* x1, uint32_t k, size_t count, uint64_t* out);
/* Merkle tree over n leaf digests with `depth` hash levels (openzl-crypto/src/merkle_tree, one H for join_leaves and join): level 0 = the n leaves, level k
 * has ceil(n / 2^k) nodes, node(k, j) = H(node(k-1, 2j), node(k-1, 2j+1)) where an absent right child reads as the zero digest.  A node whose subtree holds no
 * leaf is absent -- zero when read as a sibling, NOT H(0, 0): the reference's Default::default() rule (merkle_tree/node.rs:55-73, path.rs:405-454).  The root
 * is the one node of level `depth` (n == 0: the zero digest).  Nodes are stored level after level from level 0: zl_poseidon_merkle_nodes(n, depth) elements
 * (0 for a depth outside 1..40 or n > 2^depth).  Levels of at most ZL_TUNE_POSEIDON_TAIL nodes are finished by ONE workgroup in one launch (0: a launch per level). */
size_t zl_poseidon_merkle_nodes(size_t n, unsigned depth);
int zl_poseidon_merkle_build_dev(zl_ctx* ctx, zl_curve_t curve, const void* d_leaves, size_t n, unsigned depth, void* d_nodes, uint64_t* root_out);
/* the same from host leaves into a host node array / to the root alone (device scratch of the call is freed before it returns) */
int zl_poseidon_merkle_build(zl_ctx* ctx, zl_curve_t curve, const uint64_t* leaves, size_t n, unsigned depth, uint64_t* nodes, uint64_t* root);
int zl_poseidon_merkle_root(zl_ctx* ctx, zl_curve_t curve, const uint64_t* leaves, size_t n, unsigned depth, uint64_t* root);
/* paths[i] = the `depth` sibling digests of leaf indices[i] from the bottom up: entry 0 is the reference's Path::sibling_digest, the rest its inner_path
 * (path.rs:628-636); absent siblings are zero.  An index >= n is ZL_EINVAL before any work.  indices and paths are host memory; _dev gathers from a node
 * array in device memory, the other form from one in host memory (a plain gather: no ctx). */
int zl_poseidon_merkle_paths_dev(zl_ctx* ctx, zl_curve_t curve, const void* d_nodes, size_t n, unsigned depth, const uint64_t* indices, size_t count,
                                 uint64_t* paths);
int zl_poseidon_merkle_paths(const uint64_t* nodes, size_t n, unsigned depth, const uint64_t* indices, size_t count, uint64_t* paths);
/* roots[i] = the fold of paths[i] (depth elements) over leaves[i]: at level k the running digest joins on the right when bit k of indices[i] is set, on the
 * left otherwise (Parity::join); one lane per path, `depth` dependent hashes each.  An index >= 2^depth is ZL_EINVAL.  Host pointers. */
int zl_poseidon_merkle_roots_from_paths(zl_ctx* ctx, zl_curve_t curve, const uint64_t* leaves, const uint64_t* indices, const uint64_t* paths, unsigned depth,
                                        size_t count, uint64_t* roots);
/* ---- Merkle membership in circuit: the reference's PathVar::verify_digest with the digest itself as the leaf (openzl-crypto/src/merkle_tree/path.rs:942-1126),
 * folded with ConditionalSwap = two conditionally_selects per level (plugins/arkworks/src/constraint/mod.rs:354-390) over Boolean witnesses (mod.rs:242-258).
 * Public input: the root.  Witnesses, LEVEL-major (the reference allocates all bits, then all digests, up front; level-major lets a device lane write its row
 * front to back): the leaf, then for level j = 0..depth-1 the sibling path[j], the Boolean b_j = bit j of index (row (1 - b) b = 0), left = select(b, sib, cur),
 * right = select(b, cur, sib) (row b (t - f) = out - f each), and the 234 S-box witnesses of cur = H(left, right); the last row is cur = root.
 * Shape (n_instance, n_witness, n_constraints) = (2, 1 + 238 depth, 237 depth + 1).  depth outside 1..40, index >= 2^depth, a null pointer or an unknown curve:
 * ZL_EINVAL.  _witness: the same circuit run by a witness-only compiler (see zl_circuit_poseidon_chain_witness); Boolean and select always allocate, so the two
 * compilers' assignments are equal word for word. */
int zl_circuit_poseidon_merkle(zl_curve_t curve, unsigned depth, const uint64_t* leaf, uint64_t index, const uint64_t* path, zl_circuit** out);
int zl_circuit_poseidon_merkle_witness(zl_curve_t curve, unsigned depth, const uint64_t* leaf, uint64_t index, const uint64_t* path, zl_circuit** out);
/* The complete ASSIGNMENT of zl_circuit_poseidon_merkle(curve, depth, leaves[i], indices[i], paths[i]) per membership, one device lane each (k_pos_merkle_trace):
 *   [0] = 1   [1] = root   [2] = leaf   level j at 3 + 238 j: [+0] sibling  [+1] b_j (0 or 1)  [+2] left  [+3] right  [+4 .. +238) the 234 records of H(left, right)
 * zl_poseidon_merkle_assignment_elems(depth) = 3 + 238 depth elements (0 for a depth outside 1..40).  indices are HOST memory in every form, as in
 * zl_poseidon_merkle_paths_dev; an index >= 2^depth (>= n in the member form) is ZL_EINVAL before any work.  The host-pointer form writes count dense rows and
 * follows the common rules of the batched Poseidon entry points (ctx == NULL or a count below ZL_TUNE_POSEIDON_DEV_MIN: the host mirror over the host pool;
 * staged in chunks of ZL_TUNE_POSEIDON_CHUNK under the 256 MiB budget).  The _dev forms never take the host path (ctx == NULL is ZL_EINVAL): row i starts at
 * d_out + i * stride_elems elements, stride_elems >= the row length, elements behind the row are not written, d_out must be 16-byte aligned and must not overlap
 * the inputs.  _assignments_dev reads leaves (count elements) and paths (count x depth) from device memory; _member_assignments_dev reads both out of a node array
 * of zl_poseidon_merkle_build_dev's layout (n leaves, `depth` levels): the leaf is node (0, index), the sibling at level k node (k, (index >> k) ^ 1), zero when
 * the tree has no such node -- so [1] of every row is the tree's root. */
size_t zl_poseidon_merkle_assignment_elems(unsigned depth);
int zl_poseidon_merkle_assignments(zl_ctx* ctx, zl_curve_t curve, const uint64_t* leaves, const uint64_t* indices, const uint64_t* paths, unsigned depth, size_t count,
                                   uint64_t* out);
int zl_poseidon_merkle_assignments_dev(zl_ctx* ctx, zl_curve_t curve, const void* d_leaves, const uint64_t* indices, const void* d_paths, unsigned depth, size_t count,
                                       void* d_out, size_t stride_elems);
int zl_poseidon_merkle_member_assignments_dev(zl_ctx* ctx, zl_curve_t curve, const void* d_nodes, size_t n, unsigned depth, const uint64_t* indices, size_t count,
                                              void* d_out, size_t stride_elems);
/* ---- in circuit at every arity of the table: the reference's Spec<F, ARITY> (plugins/arkworks/src/poseidon/mod.rs:225-322).  S(a) = 8 (a + 1) + partial - 1 =
 * 78, 86, 95, 103 is the number of S-boxes one arity-a hash allocates: every S-box of the permutation in round order, lane order within a round, each as x^2,
 * x^4, x^5, except lane 0 of round 0, whose input -- the domain tag 2^a - 1 plus a round key -- is a constant the circuit folds.  3 S(a) = 234, 258, 285, 309
 * record elements; the rule of the arity-2 gadget, at width a + 1.
 * zl_circuit_poseidon_hash: ONE hash of `arity` inputs (in: arity x 4 u64).  Public input: the digest.  Witnesses: the inputs, then the 3 S(a) records; the
 *   last row is digest = public input.  Shape (n_instance, n_witness, n_constraints) = (2, a + 3 S(a), 3 S(a) + 1).  At arity 2 this is the circuit of
 *   zl_circuit_poseidon_chain(curve, 1, in, in + 4) word for word: the same matrices and the same assignment.
 * zl_circuit_poseidon_merkle_leaf: a membership whose leaf is hashed from its preimage INSIDE the circuit -- the reference's PathVar::verify,
 *   parameters.digest_with(leaf) followed by verify_digest (openzl-crypto/src/merkle_tree/path.rs:1109-1125): "I know the opening of a commitment that is in
 *   the tree".  Public input: the root.  Witnesses: the `arity` preimage elements; the 3 S(a) records of leaf = H_a(preimage) -- the leaf digest itself is a
 *   linear combination and is NOT allocated, as h_j inside a chain; then the levels exactly as zl_circuit_poseidon_merkle lays them out (sibling, Boolean bit,
 *   left, right, 234 records: arity 2 at every level).  Shape (2, a + 3 S(a) + 238 d, 3 S(a) + 237 d + 1).
 * arity outside 2..5, depth outside 1..40, index >= 2^depth, an element >= r, a null pointer or an unknown curve: ZL_EINVAL.  _witness: the same circuits run by
 * a witness-only compiler (see zl_circuit_poseidon_chain_witness); the two compilers' assignments are equal word for word.
 * SHAPES.  Four families now share n_instance == 2: chain(k) (2 + 234 k, 234 k + 1), membership(d) (1 + 238 d, 237 d + 1), hash(a) and leaf(a, d) above.
 * n_witness - n_constraints is 1, d, a - 1 and a - 1 + d.  hash(a) against chain(k): a = 2, then 236 = 2 + 234 k gives k = 1 -- the ONE coincidence, and there the
 * circuits are identical, so keys of either serve both provers.  hash against membership: d = a - 1, and a + 3 S(a) = 236, 261, 289, 314 is never 1 + 238 (a - 1)
 * = 239, 477, 715, 953.  leaf against chain: a - 1 + d >= 2.  leaf(a, d) against membership(d'): d' = a - 1 + d, which needs a + 3 S(a) = 1 + 238 (a - 1) again.
 * leaf(a, d) against leaf(a', d') or hash(a') (take d' = 0): equal differences give d - d' = a' - a, equal witness counts then need (a' + 3 S(a')) - (a + 3 S(a))
 * = 238 (a' - a), but those values lie within 314 - 236 = 78 of each other, so a' = a and d' = d.  So every prover below refuses the keys of every other
 * family, chain(1) / hash(2) apart. */
int zl_circuit_poseidon_hash(zl_curve_t curve, unsigned arity, const uint64_t* in, zl_circuit** out);
int zl_circuit_poseidon_hash_witness(zl_curve_t curve, unsigned arity, const uint64_t* in, zl_circuit** out);
int zl_circuit_poseidon_merkle_leaf(zl_curve_t curve, unsigned arity, unsigned depth, const uint64_t* preimage, uint64_t index, const uint64_t* path, zl_circuit** out);
int zl_circuit_poseidon_merkle_leaf_witness(zl_curve_t curve, unsigned arity, unsigned depth, const uint64_t* preimage, uint64_t index, const uint64_t* path,
                                            zl_circuit** out);
/* The complete ASSIGNMENTS of the two circuits, one device lane per row (k_pos_hash_trace / k_pos_leaf_merkle_trace), word for word what both compilers export:
 *   hash row:             [0] = 1   [1] = digest   [2 .. 2 + a) the inputs    then the 3 S(a) records
 *   leaf-membership row:  [0] = 1   [1] = root     [2 .. 2 + a) the preimage  the 3 S(a) records of the leaf hash   level j at 2 + a + 3 S(a) + 238 j, laid
 *                         out as in zl_poseidon_merkle_assignments: [+0] sibling  [+1] b_j  [+2] left  [+3] right  [+4 .. +238) the records of H(left, right)
 * zl_poseidon_hash_assignment_elems(arity) = 2 + a + 3 S(a) = 238, 263, 291, 316; zl_poseidon_merkle_leaf_assignment_elems(arity, depth) = that + 238 depth; 0
 * for a parameter out of range.  At arity 2 the hash rows are zl_poseidon_chain_assignments' for k = 1 byte for byte.  in / preimages: count x arity elements;
 * paths: count x depth; indices are HOST memory in every form.  The host-pointer forms write count dense rows under the common rules of the batched Poseidon
 * entry points (ctx == NULL or a count below ZL_TUNE_POSEIDON_DEV_MIN: the host mirror over the host pool; staged in chunks of ZL_TUNE_POSEIDON_CHUNK under
 * the 256 MiB budget; finished on return; an element >= r is ZL_EINVAL through the flag word).  The _dev forms never take the host path (ctx == NULL is
 * ZL_EINVAL): row i starts at d_out + i * stride_elems elements, stride_elems >= the row length, elements behind the row are not written, d_out must be 16-byte
 * aligned and must not overlap the inputs.  An index >= 2^depth (>= n in the member form) is ZL_EINVAL before any work.
 * _member_assignments_dev reads a node array of zl_poseidon_merkle_build_dev's layout (n leaves, `depth` levels) and the n x arity preimages of its leaves,
 * preimage of leaf i at element i * arity of d_preimages: the siblings as in zl_poseidon_merkle_member_assignments_dev, so [1] of every row is the tree's root.
 * An item whose H_a(preimage) differs from node (0, index) makes the call ZL_EINVAL (a second bit of the flag word): without the comparison the call would
 * quietly write a valid row for ANOTHER root. */
size_t zl_poseidon_hash_assignment_elems(unsigned arity);
size_t zl_poseidon_merkle_leaf_assignment_elems(unsigned arity, unsigned depth);
int zl_poseidon_hash_assignments(zl_ctx* ctx, zl_curve_t curve, unsigned arity, const uint64_t* in, size_t count, uint64_t* out);
int zl_poseidon_hash_assignments_dev(zl_ctx* ctx, zl_curve_t curve, unsigned arity, const void* d_in, size_t count, void* d_out, size_t stride_elems);
int zl_poseidon_merkle_leaf_assignments(zl_ctx* ctx, zl_curve_t curve, unsigned arity, const uint64_t* preimages, const uint64_t* indices, const uint64_t* paths,
                                        unsigned depth, size_t count, uint64_t* out);
int zl_poseidon_merkle_leaf_assignments_dev(zl_ctx* ctx, zl_curve_t curve, unsigned arity, const void* d_preimages, const uint64_t* indices, const void* d_paths,
                                            unsigned depth, size_t count, void* d_out, size_t stride_elems);
int zl_poseidon_merkle_leaf_member_assignments_dev(zl_ctx* ctx, zl_curve_t curve, unsigned arity, const void* d_nodes, const void* d_preimages, size_t n, unsigned depth,
                                                   const uint64_t* indices, size_t count, void* d_out, size_t stride_elems);
/* ---- Merkle forest: `trees` (1 .. 65 536) growing trees in ONE allocation -- the reference's accumulator, trees that grow by push / extend
 * (openzl-crypto/src/merkle_tree/tree.rs:287-345, 899-915) held as a fixed array with every leaf routed to one of them (forest.rs:30-40, 245-251, 465-565).
 * Every tree has `depth` (1 .. 40) hash levels and room for `capacity` leaves (1 <= capacity <= 2^depth), over the arity-2 H and the rules of the Merkle family
 * above: an absent right child is zero, a node with no leaf under it is zero (not H(0, 0)), the root is the node of level `depth`, zero for an empty tree.
 * LAYOUT: tree t occupies S = zl_poseidon_merkle_nodes(capacity, depth) elements at element offset t * S; inside a tree the layout is that of
 * zl_poseidon_merkle_build_dev for n = CAPACITY, whatever the tree's length.  The allocation is zero-filled at creation and only ever written where a leaf lies
 * below.  So every _dev entry point above that takes (d_nodes, n, depth) -- zl_poseidon_merkle_paths_dev, zl_poseidon_merkle_member_assignments_dev,
 * zl_groth16_prove_merkle_members -- works on ONE tree of the forest when called with zl_merkle_forest_tree_nodes(f, t) and n = capacity (they then accept an
 * index up to the capacity; an index at or past the tree's length names an empty slot).  The trees' lengths live on the host.
 * ctx == NULL: the HOST MIRROR -- the same layout in host memory, the same results byte for byte, updates through the host permutation over the host pool, no
 * device opened.  Otherwise the ctx must outlive the forest (a fork of a ctx serves as well); work is issued on its stream (zl_ctx_set_stream is honoured)
 * and has finished when a call returns.  One caller at a time per forest.  Staging goes through the ctx's Poseidon scratch under its 256 MiB budget and
 * ZL_TUNE_POSEIDON_CHUNK (also the lanes of one launch); the node allocation is the forest's own.  An allocation that fails is ZL_ENOMEM, nothing leaked.
 * _append: leaf i goes to tree tree_of[i], behind the leaves that tree already has, in input order (forest.rs push, leaf by leaf); then, level by level, ONE
 *   launch hashes the parents of every touched tree that have a new leaf under them -- `depth` dependent permutations per append, however many trees it touches.
 *   Checked on the host before any work: a tree id >= trees, an append that would take a tree past `capacity`, a host leaf >= r: ZL_EINVAL.  _append_dev reads the
 *   leaves from DEVICE memory (count x 4 u64) and validates them in a pass of its own before the first node is written; a host-mirror forest is ZL_EINVAL there.
 *   A refused append of either form leaves lengths and nodes exactly as they were.  count == 0: ZL_OK.
 * _roots: trees x 4 u64.  _paths: the `depth` siblings of leaf indices[i] of tree tree_of[i], as zl_poseidon_merkle_paths on a fresh build of that tree's
 *   leaves; an index >= that tree's length is ZL_EINVAL.  _tree_nodes: the address of tree t's node array (device memory; host memory for the mirror).
 * _download: one tree's S elements.  _member_assignments_dev: row i = the row zl_poseidon_merkle_member_assignments_dev writes for leaf indices[i] of tree
 *   tree_of[i] (word for word; d_out, stride_elems as there); host-mirror forest: ZL_EINVAL.  tree_of and indices are host memory everywhere. */
int zl_merkle_forest_create(zl_ctx* ctx, zl_curve_t curve, uint32_t trees, unsigned depth, size_t capacity, zl_merkle_forest** out);
void zl_merkle_forest_destroy(zl_merkle_forest* f); /* NULL is a no-op */
int zl_merkle_forest_describe(const zl_merkle_forest* f, uint32_t* trees, unsigned* depth, size_t* capacity, size_t* tree_stride_elems); /* a NULL output is skipped */
int zl_merkle_forest_lens(const zl_merkle_forest* f, uint64_t* lens);
int zl_merkle_forest_append(zl_merkle_forest* f, const uint32_t* tree_of, const uint64_t* leaves, size_t count);
int zl_merkle_forest_append_dev(zl_merkle_forest* f, const uint32_t* tree_of, const void* d_leaves, size_t count);
int zl_merkle_forest_roots(const zl_merkle_forest* f, uint64_t* roots);
int zl_merkle_forest_paths(const zl_merkle_forest* f, const uint32_t* tree_of, const uint64_t* indices, size_t count, uint64_t* paths);
int zl_merkle_forest_tree_nodes(const zl_merkle_forest* f, uint32_t tree, const void** nodes);
int zl_merkle_forest_download(const zl_merkle_forest* f, uint32_t tree, uint64_t* nodes);
int zl_merkle_forest_member_assignments_dev(const zl_merkle_forest* f, const uint32_t* tree_of, const uint64_t* indices, size_t count, void* d_out, size_t stride_elems);
/* Groth16::compile with rng = SplitMix64(seed): trapdoor setup, proving key generated on the device */
int zl_groth16_compile(zl_ctx* ctx, const zl_circuit* c, uint64_t seed, zl_g16_keys** out);
int zl_groth16_keys_trapdoor(const zl_g16_keys* k, uint64_t* out20); /* alpha, beta, gamma, delta, tau (canonical) */
/* Groth16::prove with rng = SplitMix64(seed); r_out / s_out (optional) receive the sampled blinding scalars */
int zl_groth16_prove_circuit(zl_ctx* ctx, const zl_g16_keys* k, const zl_circuit* c, uint64_t seed, zl_g16_proof* proof,
                             uint64_t* r_out, uint64_t* s_out);

/* A STREAM of proofs over one key: proofs[i] = Groth16::prove(keys, *circuits[i], SplitMix64(seeds[i])), i < count, issued from two host threads over two
 * prover lanes (ctx itself and a fork of it that the ctx keeps for later calls) -- the proofs are the ones `count` calls of zl_groth16_prove_circuit return,
 * byte for byte, at the throughput of two lanes (958 465 constraints: 17.7 instead of 18.8 ms per proof; 14 977: 2.35 instead of 3.05; 235: 0.9 instead of
 * 1.5).  ctx must be the root ctx the keys live on and the keys must be bound to their circuit (compiled here, or proven once after decoding); circuits may
 * repeat.  The first failure is returned and the remaining proofs are not started.  The kept lane is the library's own fork and pins nothing once the call
 * has returned: zl_bases_free / zl_bases_precompute / zl_r1cs_free on the ctx release it first when it is idle (round 6; forks the CALLER made with
 * zl_ctx_fork still pin the parent's handles).  zl_ctx_drop_lanes(ctx) releases it explicitly (zl_ctx_destroy does too); it returns ZL_EINVAL while a call is
 * using the lane. */
int zl_groth16_prove_circuits(zl_ctx* ctx, const zl_g16_keys* k, const zl_circuit* const* circuits, const uint64_t* seeds, size_t count, zl_g16_proof* proofs);
int zl_ctx_drop_lanes(zl_ctx* ctx);
/* e(P, Q) in GT after the final exponentiation: 12 canonical Fq coefficients (BLS12-381: 12 x 6 u64, BN254: 12 x 4 u64) of the
 * polynomial in w, Fq12 = Fq[w]/(w^12 - 2 w^6 + 2) (BLS12-381) or (w^12 - 18 w^6 + 82) (BN254) */
int zl_pairing(zl_curve_t curve, const uint64_t* p_xy, const uint64_t* q_xy, uint64_t* out12);
/* prod_i e(P_i, Q_i) after ONE final exponentiation: 12 canonical Fq coefficients, exactly what zl_pairing returns for n = 1
 * (ark_ec::PairingEngine::product_of_pairings, used by plugins/arkworks/src/pairing.rs:47-90).  ps_xy: n G1 points (x||y canonical),
 * qs_xy: n G2 points (x.c0||x.c1||y.c0||y.c1); all-zero = infinity, contributes 1.  Miller loops on the device, final exponentiation on the host.
 * ZL_ENOTCURVE when the Miller product is zero (inputs outside the pairing groups), as zl_pairing. */
int zl_pairing_product(zl_ctx* ctx, zl_curve_t curve, const uint64_t* ps_xy, const uint64_t* qs_xy, size_t n, uint64_t* out12);
/* `count` INDEPENDENT products of `pairs_each` pairings each, Miller loops AND final exponentiations on the device: what a caller of the plugin's
 * PairingEngineExt::same / same_ratio (plugins/arkworks/src/pairing.rs:47-90, ratio.rs:102-113) needs when it checks many ratios at once.  Product j runs
 * over pairs [j * pairs_each, (j + 1) * pairs_each) of ps_xy / qs_xy (layouts of zl_pairing_product); out12 + j * 12 Fq receives exactly what
 * zl_pairing_product returns for those pairs.  status (optional, count entries): ZL_OK, or ZL_ENOTCURVE for a zero Miller product (inputs outside the
 * pairing groups; the value is then zero).  A bad product is data, not a failure: the call returns ZL_OK once the batch is processed.  count == 0: ZL_OK,
 * nothing is written.  pairs_each == 0: every result is one.  pairs_each above 65 536 (the pairs of one device launch set): ZL_EINVAL, before any work.
 * The products are laid out over launch sets of floor(65 536 / pairs_each) products (fewer when ZL_TUNE_FEXP_CHUNK is set: a test knob). */
int zl_pairing_products(zl_ctx* ctx, zl_curve_t curve, const uint64_t* ps_xy, const uint64_t* qs_xy, size_t count, size_t pairs_each, uint64_t* out12,
                        int32_t* status);
/* Groth16::verify for `count` proofs against one key in one random linear combination:
 *   prod_i e(rho_i A_i, B_i) * e(-sum_i rho_i C_i, delta) * e(-sum_i rho_i IC_i, gamma) * e(-(sum_i rho_i) alpha, beta) == 1,
 * IC_i = gamma_abc[0] + sum_j x_ij gamma_abc[j+1], so the last three pairs are shared by the whole batch (count + 3 Miller loops, one final exponentiation).
 * rho_i: nonzero 128-bit scalars from SplitMix64(*seed), or from the OS (getrandom) when seed == NULL.  A seed the prover can predict voids soundness:
 * pass NULL in production.  public_inputs: count x n_public x 4 u64 canonical (each < r; otherwise ZL_EINVAL, nothing computed, outputs untouched),
 * without the leading ONE.  One value at or above r refuses the whole call, before rho is drawn: an error as in zl_groth16_verify, not a verdict.
 * *ok = 1 iff every proof verifies.  ok_each (optional, count bytes): per-proof verdicts, each equal to what zl_groth16_verify returns for that proof;
 * computed from the batch when it accepts, by per-proof products (device Miller loops, host final exponentiations) when it rejects.
 * A proof with A or B at infinity is invalid, as in zl_groth16_verify.  n_public + 1 != the key's gamma_abc length: ZL_EINVAL.  count == 0: *ok = 1.
 * rho_i A_i is formed on the device (inside the Miller loops' input kernel), sum_i rho_i C_i is a device MSM, sum_i rho_i x_ij mod r and IC on the host. */
int zl_groth16_verify_batch(zl_ctx* ctx, const zl_g16_keys* k, const uint64_t* public_inputs, size_t n_public, const zl_g16_proof* proofs,
                            size_t count, const uint64_t* seed, int* ok, uint8_t* ok_each);

/* ---- wire formats: arkworks 0.3 CanonicalSerialize, compressed (replaces proof_as_bytes / HasSerialization,
 * /root/reference/plugins/arkworks/src/groth16.rs:68-107).  x little-endian, flags in the top two bits of the last byte
 * (bit 7: y is the larger root, bit 6: infinity); Fq2: c0 then c1 (flags on c1).  Proof = A || B || C: 192 bytes (BLS12-381) / 128 (BN254).
 * Host only.  NOT verified against arkworks-produced bytes (the reference holds no vector): pinned to an independent restatement
 * (oracle/pyoracle.py) and round trips.  from_bytes: ZL_EINVAL = malformed, ZL_ENOTCURVE = no such point / outside the subgroup. */
size_t zl_point_bytes(zl_curve_t curve, zl_group_t group);
int zl_point_to_bytes(zl_curve_t curve, zl_group_t group, const uint64_t* xy, uint8_t inf, uint8_t* out);
int zl_point_from_bytes(zl_curve_t curve, zl_group_t group, const uint8_t* in, uint64_t* xy, uint8_t* inf);
/* The same decoding for a batch ON THE DEVICE, one lane per point (openzl_amd/csrc/zl_decode_dev.hip): the square root(s), the sign rule and the
 * subgroup check (a plain multiplication by r; BN254 G1 has cofactor 1 and needs none).  in: count packed records of zl_point_bytes(curve, group) bytes, at
 * any byte alignment.  status[i], out_xy + i x (2 or 4 Fq of canonical words) and out_inf[i] are what zl_point_from_bytes returns for record i: all-zero
 * words and inf = 0 on every status but ZL_OK.  Returns ZL_OK when the batch was processed (bad records are data, not a call failure), ZL_EINVAL for bad
 * arguments, ZL_EHIP / ZL_ENOMEM as elsewhere.  count == 0 is ZL_OK. */
int zl_points_from_bytes_batch(zl_ctx* ctx, zl_curve_t curve, zl_group_t group, const uint8_t* in, size_t count, uint64_t* out_xy, uint8_t* out_inf,
                               int32_t* status);
/* count proofs of zl_groth16_proof_bytes(curve) bytes each, decoded on the device.  status[i] and proofs[i] are what zl_groth16_proof_from_bytes returns and
 * leaves for record i: the status of the first failing point of A, B, C; that point and those behind it all-zero, the points in front of it decoded
 * (a caller looks at the status first, as with the host function). */
int zl_groth16_proofs_from_bytes_batch(zl_ctx* ctx, zl_curve_t curve, const uint8_t* in, size_t count, zl_g16_proof* proofs, int32_t* status);
/* zl_groth16_verify_batch over wire proofs: the records are decoded on the device (as above), then the proofs that decoded go through the random linear
 * combination of zl_groth16_verify_batch with their public inputs.  ok_each[i] (optional) = 1 iff record i decodes AND verifies, i.e. what
 * zl_groth16_proof_from_bytes followed by zl_groth16_verify gives; *ok = 1 iff every record does; status (optional, count codes) = the decode statuses.
 * public_inputs, n_public, seed: as zl_groth16_verify_batch (n_public + 1 != the key's gamma_abc length: ZL_EINVAL; count == 0: *ok = 1).  public_inputs
 * are canonical (each < r; otherwise ZL_EINVAL, nothing computed, outputs untouched): all count x n_public values are checked ahead of the decoder, those
 * of a record that would not decode included, and status is among the outputs left untouched. */
int zl_groth16_verify_batch_bytes(zl_ctx* ctx, const zl_g16_keys* k, const uint64_t* public_inputs, size_t n_public, const uint8_t* proofs_bytes,
                                  size_t count, const uint64_t* seed, int* ok, uint8_t* ok_each, int32_t* status);
/* Uncompressed form (ark's serialize_uncompressed / serialize_unchecked): x then y, flags on the last byte of y; a finite point
 * carries no flag bits, infinity is written as (0, 1) with bit 6 set.  check = 0 is deserialize_unchecked (coordinates must be canonical
 * integers, nothing else is verified); check != 0 also requires a point of the prime-order subgroup (ZL_ENOTCURVE otherwise). */
size_t zl_point_bytes_uncompressed(zl_curve_t curve, zl_group_t group);
int zl_point_to_bytes_uncompressed(zl_curve_t curve, zl_group_t group, const uint64_t* xy, uint8_t inf, uint8_t* out);
int zl_point_from_bytes_uncompressed(zl_curve_t curve, zl_group_t group, const uint8_t* in, int check, uint64_t* xy, uint8_t* inf);
/* The same bytes validated on the HOST only (no ctx, no device memory): framing, Vec lengths against the input size, canonical coordinates, flag bits, the shape
 * relations between the five queries; ZL_CHECK also verifies the verifying-key points (curve and subgroup).  ZL_OK = zl_groth16_keys_from_bytes would accept the
 * framing (its device-side curve checks of the queries under ZL_CHECK are not repeated here).  Same error codes. */
int zl_groth16_keys_parse(zl_curve_t curve, const uint8_t* in, size_t len, unsigned flags);
/* ark_groth16::VerifyingKey<E>::serialize (compressed points): alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1 (u64 length first).
 * The reference's VerifyingContext (/root/reference/plugins/arkworks/src/groth16.rs:181-396) frames a PreparedVerifyingKey as
 *     vk | alpha_g1_beta_g2 (one Fqk) | gamma_g2_neg_pc | delta_g2_neg_pc
 * where the last two are written through `<E::G2Prepared as HasSerialization>::Serialize` (groth16.rs:208-211).  HasSerialization /
 * HasDeserialization are hook traits (plugins/arkworks/src/serialize.rs:21-30) that NO file of the reference implements for any curve
 * (grep: no `impl ... HasSerialization`): the bytes of a prepared G2 point (ark-ec's Miller-loop line coefficients) are left to a
 * downstream crate, so the reference defines no layout for two of the four fields and VerifyingContext: Encode / Decode cannot even be
 * instantiated from the reference alone.  alpha_g1_beta_g2 is the pairing value ark's final exponentiation produces; this backend's
 * pairing (csrc/zl_pairing.h) takes the exact (q^12 - 1)/r power in a tower-free basis, and whether ark-ec 0.3's hard part returns that
 * power or a fixed multiple of it cannot be checked without the crate.  What IS defined and restated is the first field, vk, below; a
 * verifier built from it recomputes the other three (zl_groth16_verify does). */
int zl_groth16_vk_to_bytes(const zl_g16_keys* k, uint8_t* out, size_t cap, size_t* len);

/* ---- the embedded twisted Edwards curves and hybrid encryption (csrc/zl_edwards.h, csrc/zl_edwards_dev.hip) ----------------------------
 * The two embedded curves the reference's arkworks plugin re-exports over this backend's scalar fields: ed_on_bls12_381 (Jubjub) for ZL_BLS12_381 and ed-on-bn254
 * (Baby Jubjub) for ZL_BN254: a x^2 + y^2 = 1 + d x^2 y^2 over F_q, q = the pairing curve's r, subgroup order l, cofactor 8.  Both are complete: the identity
 * is the ordinary point (0, 1) and there is no point at infinity.  The constants are the published parameters of the two arkworks crates; they are not compared
 * with arkworks bytes -- the reference holds no vectors for these curves.  The generator is not a constant: the reference's DiffieHellman carries it as a
 * field (openzl-crypto/src/algebra/diffie_hellman.rs), here it is an argument.
 * A point is 8 words, x then y, canonical (each below q); a scalar is 4 canonical words below l.  Strides are 0 (one operand for all items) or 1.
 * zl_ed_params: a, d, order, cofactor, 4 words each, canonical; a NULL output is skipped.  zl_ed_add / zl_ed_scalar_mul: host, one item; ZL_EINVAL for an operand
 * that is out of range or not on the curve.
 * zl_ed_scalar_mul_batch: out[i] = scalars[i * scalar_stride] * points[i * point_stride].  status[i]: 0 ok, 1 a coordinate >= q, 2 not on the curve, 3 not in
 * the prime-order subgroup (only with ZL_ED_CHECK_SUBGROUP, which adds the test l P = (0, 1): a second multiplication), 4 scalar >= l; the LOWEST code that
 * applies.  An item with a non-zero status writes (0, 1) and leaves every other item untouched.  status == NULL: any such item makes the whole call ZL_EINVAL
 * (through the flag word on the device), the outputs are then unspecified.  count == 0 is ZL_OK and writes nothing; a null required pointer, an unknown curve, an
 * unknown flag or a stride above 1 is ZL_EINVAL.  ctx == NULL or a count below ZL_TUNE_ED_DEV_MIN runs the host mirror over the host pool; otherwise the call
 * is staged in chunks of at most ZL_TUNE_ED_CHUNK items under a byte budget (one window table of 2304 B per lane lives in the ctx's scratch) and has finished on
 * return.  A shared point (point_stride == 0) takes the fixed-base kernel from ZL_TUNE_ED_FIXED_MIN items; a shared scalar reads its digits wave-uniformly.
 * Results are byte-identical on every path.  The _dev form takes DEVICE pointers for points, scalars, out and status (never the host path: ctx == NULL is
 * ZL_EINVAL); with a shared point on the fixed-base path it copies that one point to the host on the ctx's stream and waits for it, because the table is built
 * on the host.
 * Hybrid encryption: the reference's encryption::hybrid::Hybrid<DiffieHellman, FixedDuplexer>.  Encrypt: epk_i = esk_i G, S_i = esk_i pk_i (GenerateSecret),
 * then the duplex cipher above under the key (S_i.x, S_i.y), key_len = 2 -- the reference leaves group -> key to the caller's converter
 * (openzl-crypto/src/encryption/convert/key.rs); here it is the two affine coordinates.  Decrypt: S_i = sk epk_i (ReconstructSecret), then the duplex
 * decryption and its tag verdict; sk_stride == 0 is the scan of a ledger with one key.  Width, header_len, blocks, initial_state and the element range of
 * headers, texts and tags are the duplex call's, with its ZL_EINVAL.  status[i] as above (encrypt: of pk_i, esk_i and the generator; decrypt: of epk_i and
 * sk).  An item with a non-zero status has epk = (0, 1) (encrypt) and ok_each[i] = 0 (decrypt); its texts and tag are computed from some key and are
 * unspecified.  Decryption never fails the batch for such an item -- ledger data is untrusted -- and status may be NULL there; encryption with status == NULL
 * returns ZL_EINVAL for one.  On the device the shared secrets stay in the ctx's scratch and the duplex kernel reads them there: no bus round trip.  The _dev
 * forms take DEVICE pointers for scalars, points, headers, texts, tags and status; generator_xy, initial_state and ok_each stay host memory. */
#define ZL_ED_CHECK_SUBGROUP 1u
int zl_ed_params(zl_curve_t curve, uint64_t* a, uint64_t* d, uint64_t* order, uint64_t* cofactor);
int zl_ed_add(zl_curve_t curve, const uint64_t* p_xy, const uint64_t* q_xy, uint64_t* out_xy);
int zl_ed_scalar_mul(zl_curve_t curve, const uint64_t* p_xy, const uint64_t* k, uint64_t* out_xy);
int zl_ed_scalar_mul_batch(zl_ctx* ctx, zl_curve_t curve, const uint64_t* points_xy, size_t point_stride, const uint64_t* scalars, size_t scalar_stride, size_t count,
                           unsigned flags, uint64_t* out_xy, uint8_t* status);
int zl_ed_scalar_mul_batch_dev(zl_ctx* ctx, zl_curve_t curve, const void* d_points_xy, size_t point_stride, const void* d_scalars, size_t scalar_stride, size_t count,
                               unsigned flags, void* d_out_xy, void* d_status);
int zl_hybrid_encrypt_batch(zl_ctx* ctx, zl_curve_t curve, unsigned width, const uint64_t* initial_state, const uint64_t* generator_xy, const uint64_t* esk,
                            const uint64_t* pks_xy, size_t pk_stride, const uint64_t* headers, size_t header_len, const uint64_t* plaintexts, size_t blocks, size_t count,
                            unsigned flags, uint64_t* epks_xy, uint64_t* ciphertexts, uint64_t* tags, uint8_t* status);
int zl_hybrid_encrypt_batch_dev(zl_ctx* ctx, zl_curve_t curve, unsigned width, const uint64_t* initial_state, const uint64_t* generator_xy, const void* d_esk,
                                const void* d_pks_xy, size_t pk_stride, const void* d_headers, size_t header_len, const void* d_plaintexts, size_t blocks, size_t count,
                                unsigned flags, void* d_epks_xy, void* d_ciphertexts, void* d_tags, void* d_status);
int zl_hybrid_decrypt_batch(zl_ctx* ctx, zl_curve_t curve, unsigned width, const uint64_t* initial_state, const uint64_t* sks, size_t sk_stride, const uint64_t* epks_xy,
                            const uint64_t* headers, size_t header_len, const uint64_t* ciphertexts, const uint64_t* tags, size_t blocks, size_t count, unsigned flags,
                            uint64_t* plaintexts, uint8_t* ok_each, uint8_t* status);
int zl_hybrid_decrypt_batch_dev(zl_ctx* ctx, zl_curve_t curve, unsigned width, const uint64_t* initial_state, const void* d_sks, size_t sk_stride, const void* d_epks_xy,
                                const void* d_headers, size_t header_len, const void* d_ciphertexts, const void* d_tags, size_t blocks, size_t count, unsigned flags,
                                void* d_plaintexts, uint8_t* ok_each, void* d_status);
/* The scalar multiplication in circuit (host compilers): "the public point Q is s P for the public point P and a secret scalar s" -- what the reference's
 * DiffieHellman<S, G> runs under a compiler in derive, agree, generate_secret and reconstruct_secret.  The gadget (csrc/zl_host.h, namespace edwards) follows
 * r1cs-std's affine twisted-Edwards variable and its default double-and-add scalar_mul_le; it is restated from the published formulas and NOT compared with
 * arkworks matrices: the reference holds none.  1 <= bits <= the bit length of l (252 for ZL_BLS12_381, 251 for ZL_BN254); s < 2^bits and s < l.
 * Public inputs: P.x, P.y, Q.x, Q.y.  Witnesses: s, its bits b_0 .. b_{bits-1} (Boolean, least significant first), then R_1 = (select(b_0, P.x, 0),
 * select(b_0, P.y, 1)), then per step i = 1 .. bits - 1 thirteen records: xy, xx, yy, M.x, M.y of M_i = 2 M_{i-1} (M_0 = P; (a xx + yy) M.x = 2 xy,
 * (2 - a xx - yy) M.y = yy - a xx), u, v0, v1, w, T.x, T.y of T = R_i + M_i (u = (y1 - a x1)(x2 + y2), v0 = x1 y2, v1 = x2 y1, w = v0 v1,
 * (1 + d w) T.x = v0 + v1, (1 - d w) T.y = u + a v0 - v1), and R_{i+1} = (select(b_i, T.x, R_i.x), select(b_i, T.y, R_i.y)).  Rows: one per bit, sum 2^i b_i
 * = s, one per record, Q.x and Q.y bound last.  SHAPE, derived again: n_instance = 1 + 4; n_witness = 1 + bits + 2 + 13 (bits - 1) = 14 bits - 10;
 * n_constraints = bits + 1 + 2 + 13 (bits - 1) + 2 = 14 bits - 8: 3 520 rows on Jubjub and 3 506 on Baby Jubjub at full width.  P is a public input: the
 * verifier checks that it is on the curve, the circuit does not.  n_instance = 5 cannot be an encryption's shape either: that family has K = n_witness -
 * (n_constraints - 1) >= 1, here it is -1 (tests/test_ed_circuit_host.py repeats the arithmetic); every other family has n_instance = 2.
 * _witness: the same circuit in the witness-only compiler, assignments equal word for word.  zl_circuit_witness_only_compatible: 1 when a FULL compiler
 * folded constants the way a witness-only run of the same circuit code will (it holds for every circuit of this header), else 0.
 * ZL_EINVAL: an unknown curve, bits out of range, a coordinate >= q, a point off the curve, a scalar >= l or >= 2^bits, a null pointer.
 * The complete ASSIGNMENTS, one device lane per row (k_ed_mul_trace: the ladder in extended coordinates, one inversion a lane, the affine records by
 * Montgomery's trick), word for word what both compilers export:
 *   [0] = 1   [1 .. 5) P, Q   [5] s   [6 .. 6 + bits) the bits   then R_1   then the 13 records of every step in the order above
 * zl_ed_scalar_mul_assignment_elems = 14 bits - 5; 0 for a parameter out of range.  The host-pointer form writes count dense rows: ctx == NULL or a count below
 * ZL_TUNE_ED_DEV_MIN runs the byte-identical host mirror over the host pool; otherwise staged in chunks of ZL_TUNE_ED_CHUNK rows under the 256 MiB budget (a row
 * at full width is about 113 KB: some 2 300 rows a chunk); finished on return; an item the circuit would refuse is ZL_EINVAL through the flag word.  The _dev
 * form takes DEVICE pointers and never the host path (ctx == NULL is ZL_EINVAL): row i starts at d_out + i * stride_elems elements, stride_elems >= the row
 * length, elements behind the row are not written, d_out must be 16-byte aligned and must not overlap the inputs.  point_stride is 0 (one point for all) or 1.
 * zl_groth16_prove_ed_scalar_muls: from HOST points and scalars to proofs -- proofs[j] is byte for byte what zl_groth16_prove_resident returns for row j with
 * (r[j], s[j]); results_out (count x 8 words, may be NULL) receives Q; the multiplication runs ONCE.  The resident circuit must have the shape (5, 14 bits - 10,
 * 14 bits - 8), else ZL_EINVAL; error order and dispatch bounds are zl_groth16_prove_batch's and are not moved: bits <= 146 has a domain of at most 2^11 and takes
 * the device batch path from 64 proofs, full width (2^12) loops the resident prover over rows staged at most 64 MiB at a time. */
int zl_circuit_ed_scalar_mul(zl_curve_t curve, unsigned bits, const uint64_t* point_xy, const uint64_t* scalar, zl_circuit** out);
int zl_circuit_ed_scalar_mul_witness(zl_curve_t curve, unsigned bits, const uint64_t* point_xy, const uint64_t* scalar, zl_circuit** out);
int zl_circuit_witness_only_compatible(const zl_circuit* c); /* 1 / 0 */
size_t zl_ed_scalar_mul_assignment_elems(zl_curve_t curve, unsigned bits);
int zl_ed_scalar_mul_assignments(zl_ctx* ctx, zl_curve_t curve, unsigned bits, const uint64_t* points_xy, size_t point_stride, const uint64_t* scalars, size_t count,
                                 uint64_t* out);
int zl_ed_scalar_mul_assignments_dev(zl_ctx* ctx, zl_curve_t curve, unsigned bits, const void* d_points_xy, size_t point_stride, const void* d_scalars, size_t count,
                                     void* d_out, size_t stride_elems);
int zl_groth16_prove_ed_scalar_muls(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, unsigned bits, const uint64_t* points_xy, size_t point_stride,
                                    const uint64_t* scalars, const uint64_t* r, const uint64_t* s, size_t count, zl_g16_proof* proofs, uint64_t* results_out);
/* The hybrid encryption in circuit (host compilers): "this ciphertext is the hybrid encryption, to the public key pk, of a plaintext I know" -- what the
 * reference's encryption::hybrid::Hybrid<DiffieHellman, FixedDuplexer>::encrypt (openzl-crypto/src/encryption/hybrid.rs, impl Encrypt) runs under a compiler:
 * epk = derive_ephemeral(esk) = esk G, S = generate_secret(pk, esk) = esk pk, then the base cipher under S -- here zl_circuit_poseidon_encrypt's duplex with the
 * key (S.x, S.y), key_len = 2, the convention zl_hybrid_encrypt_batch fixed.  It JOINS the two circuits above: the cipher's key variables ARE the pk ladder's
 * output, which two separate proofs could not bind.  width 3..6 (rate = width - 1), 1 <= bits <= the bit length of l, header_len H <= 64, blocks N in 1..1024,
 * initial_state NULL = zero; T = N rate.
 * Public inputs, after the leading 1 (Ciphertext::extend: epk, then the base ciphertext = tag, then message): G.x G.y, pk.x pk.y, epk.x epk.y, tag, the T
 * ciphertext elements, the H header elements.  G and pk are public variables, as P is above: the verifier checks that they are the generator and on the curve,
 * the circuit does not; no in-circuit subgroup test.  Every operand of a product stays a variable: zl_circuit_witness_only_compatible is 1.
 * Witnesses: esk; its `bits` Boolean bits, least significant first, allocated ONCE and shared by both ladders; the ladder over G -- R_1, then 13 records per step
 * exactly as in zl_circuit_ed_scalar_mul; the ladder over pk in the same form, whose last R is S: bound to nothing public, it is the cipher's key; the T
 * plaintext elements; the 3 S records of the cipher as zl_circuit_poseidon_encrypt orders them at K = 2, S = (F - 1 - Z) + (SB + N - 1) F with Z = max(0,
 * rate - 2).  Rows: one per bit, sum 2^i b_i = esk, the G ladder's 2 + 13 (bits - 1), epk.x and epk.y bound, the pk ladder's, the cipher's 3 S, tag = public tag,
 * one per ciphertext element.
 * SHAPE, derived again: n_instance = 1 + 7 + T + H = 8 + T + H; n_witness = 1 + bits + 2 (13 bits - 11) + T + 3 S = 27 bits - 21 + T + 3 S; n_constraints =
 * bits + 1 + (13 bits - 11) + 2 + (13 bits - 11) + 3 S + 1 + T = 27 bits - 18 + 3 S + T (27 bits - 19 rows in front of the cipher's 3 S + 1 + T); assignment
 * row length 27 bits - 13 + 2 T + H + 3 S.  FAMILIES: n_witness - (n_constraints - 1) = -2 and n_instance >= 10 here; the scalar multiplications have -1 and 5, the
 * encryptions K >= 1, every other family n_instance = 2: no other family's keys pass this family's shape check and these keys pass no other's.  WITHIN the
 * family the shape fixes T + H and 27 bits + T + 3 S and does not separate bits from S: distinct tuples of one shape are different circuits of one shape, as
 * the encryption family's one pair is; tests/test_hybrid_circuit_host.py walks the tuples within the limits and records which collide.
 * _witness: the same circuit in the witness-only compiler, assignments equal word for word.
 * ZL_EINVAL: an unknown curve, a parameter out of range, a coordinate >= q, G or pk off the curve, esk >= l or >= 2^bits, a header, plaintext or initial-state
 * element >= r, a null pointer.
 * The complete ASSIGNMENTS, word for word what both compilers export:
 *   [0] = 1  [1..3) G  [3..5) pk  [5..7) epk  [7] tag  [8 .. 8 + T) ciphertext  [.. + H) header  esk  the bits  the G ladder  the pk ladder  plaintext  records
 * On the device a chunk is TWO launches on one stream: k_ed_hybrid_ladders, one lane per (row, ladder) -- the two ladders depend only on esk's bits, and a lane
 * running both in series would pay the latency twice -- and k_pos_duplex_trace_in, the cipher keyed from the row's own S cells.
 * zl_hybrid_encrypt_assignment_elems: the row length; 0 for a parameter out of range.  The host-pointer form writes count dense rows; generator_xy is ONE host
 * point for the call, pk_stride 0 (one key for all) or 1; count == 0 is ZL_OK; ctx == NULL or a count below ZL_TUNE_ED_DEV_MIN runs the byte-identical host mirror
 * over the host pool; otherwise staged in chunks of ZL_TUNE_ED_CHUNK rows under the 256 MiB budget of the embedded-curve unit's slot; finished on return; an
 * item the circuit would refuse is ZL_EINVAL through the flag word; G and initial_state are checked on the host before any work.  The _dev form takes DEVICE
 * pointers for esk, pks, headers, plaintexts and d_out and never the host path (ctx == NULL is ZL_EINVAL): row i starts at d_out + i * stride_elems elements,
 * stride_elems >= the row length, elements behind the row are not written, d_out must be 16-byte aligned and must not overlap the inputs.
 * zl_groth16_prove_hybrid_encryptions: from HOST inputs to proofs -- proofs[j] is byte for byte what zl_groth16_prove_resident returns for row j with (r[j],
 * s[j]); epks_out (count x 8 words), tags_out (count x 4) and ciphertexts_out (count x T x 4), each may be NULL; the agreement and the cipher run ONCE.  The
 * resident circuit must have the shape above, else ZL_EINVAL; error order and dispatch bounds are zl_groth16_prove_batch's and are not moved; off the device
 * batch path the rows come through host staging of at most 64 MiB at a time. */
int zl_circuit_hybrid_encrypt(zl_curve_t curve, unsigned width, unsigned bits, const uint64_t* initial_state, const uint64_t* generator_xy, const uint64_t* esk,
                              const uint64_t* pk_xy, const uint64_t* header, size_t header_len, const uint64_t* plaintext, size_t blocks, zl_circuit** out);
int zl_circuit_hybrid_encrypt_witness(zl_curve_t curve, unsigned width, unsigned bits, const uint64_t* initial_state, const uint64_t* generator_xy, const uint64_t* esk,
                                      const uint64_t* pk_xy, const uint64_t* header, size_t header_len, const uint64_t* plaintext, size_t blocks, zl_circuit** out);
size_t zl_hybrid_encrypt_assignment_elems(zl_curve_t curve, unsigned width, unsigned bits, size_t header_len, size_t blocks);
int zl_hybrid_encrypt_assignments(zl_ctx* ctx, zl_curve_t curve, unsigned width, unsigned bits, const uint64_t* initial_state, const uint64_t* generator_xy, const uint64_t* esk,
                                  const uint64_t* pks_xy, size_t pk_stride, const uint64_t* headers, size_t header_len, const uint64_t* plaintexts, size_t blocks, size_t count,
                                  uint64_t* out);
int zl_hybrid_encrypt_assignments_dev(zl_ctx* ctx, zl_curve_t curve, unsigned width, unsigned bits, const uint64_t* initial_state, const uint64_t* generator_xy,
                                      const void* d_esk, const void* d_pks_xy, size_t pk_stride, const void* d_headers, size_t header_len, const void* d_plaintexts,
                                      size_t blocks, size_t count, void* d_out, size_t stride_elems);
int zl_groth16_prove_hybrid_encryptions(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, unsigned width, unsigned bits, const uint64_t* initial_state,
                                        const uint64_t* generator_xy, const uint64_t* esk, const uint64_t* pks_xy, size_t pk_stride, const uint64_t* headers,
                                        size_t header_len, const uint64_t* plaintexts, size_t blocks, const uint64_t* r, const uint64_t* s, size_t count,
                                        zl_g16_proof* proofs, uint64_t* epks_out, uint64_t* tags_out, uint64_t* ciphertexts_out);

/* ---- per-call device timing (HIP events on the ctx's stream) -------------------------------------------- */
typedef struct zl_timing {
    float total_ms;      /* first kernel start -> last kernel end of the last zl_msm* / zl_ntt* call */
    float dominant_ms;   /* the dominant kernel: bucket accumulation (MSM) / all butterfly passes (NTT) */
    uint32_t launches;   /* launches of the dominant kernel in that call (zl_msm_multi_dev: one accumulation launch per chunk of vectors) */
    uint32_t window_bits;
    uint64_t entries;    /* MSM: (point, window) pairs accumulated */
} zl_timing;
int zl_ctx_enable_timing(zl_ctx* ctx, int on);
int zl_last_timing(zl_ctx* ctx, zl_timing* out);

#ifdef __cplusplus
}
#endif
#endif
