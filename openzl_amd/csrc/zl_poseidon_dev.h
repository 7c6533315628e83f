// zl_poseidon_dev.h -- internal layout and limits of the batched Poseidon unit (zl_poseidon_dev.hip): the device constant table, the knob defaults and the
// Merkle node-array geometry shared by the host path, the device path and the gather.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace openzl {
namespace poseidon_dev {
// The specification table, per arity (plugins/arkworks/src/poseidon/mod.rs:300-322 states it for BN254; BLS12-381 Fr takes the same rows, as it does at arity 2):
//   arity 2 3 4 5 -> width 3 4 5 6, 8 full rounds, 55 55 56 56 partial rounds, domain tag 2^arity - 1 (openzl-crypto/src/poseidon/hash.rs:64-135).
// The host mirror (zl_host.h) and the device unit both read this one function.
struct Spec {
    unsigned arity, width, full_rounds, partial_rounds;
    uint64_t tag;
    constexpr unsigned rounds() const { return full_rounds + partial_rounds; }
    constexpr unsigned keys() const { return width * rounds(); }
};
constexpr unsigned MIN_ARITY = 2, MAX_ARITY = 5, MIN_WIDTH = MIN_ARITY + 1, MAX_WIDTH = MAX_ARITY + 1, N_WIDTHS = MAX_WIDTH - MIN_WIDTH + 1;
constexpr bool arity_ok(unsigned arity) { return arity >= MIN_ARITY && arity <= MAX_ARITY; }
constexpr bool width_ok(unsigned width) { return width >= MIN_WIDTH && width <= MAX_WIDTH; }
constexpr Spec spec(unsigned arity) { return Spec{arity, arity + 1, 8, arity <= 3 ? 55u : 56u, ((uint64_t)1 << arity) - 1}; }
constexpr Spec spec_of_width(unsigned width) { return spec(width - 1); }
static_assert(spec(2).width == 3 && spec(2).rounds() == 63 && spec(2).tag == 3 && spec(3).width == 4 && spec(3).rounds() == 63 && spec(3).tag == 7 &&
                  spec(4).width == 5 && spec(4).rounds() == 64 && spec(4).tag == 15 && spec(5).width == 6 && spec(5).rounds() == 64 && spec(5).tag == 31,
              "the reference's Spec table");
// the device table of one (curve, width): W * rounds round keys [W * round + lane], W * W MDS entries [W * row + column], the tag; entries of TAB_WORDS u32
// slots holding the nine 29-bit limbs of x R' mod r (R' = 2^261: the device multiplier's own Montgomery form).  Width 3: 189 keys, 9 MDS entries, the tag 3.
constexpr int tab_keys(unsigned) { return 0; }
constexpr int tab_mds(unsigned width) { return (int)spec_of_width(width).keys(); }
constexpr int tab_tag(unsigned width) { return tab_mds(width) + (int)(width * width); }
constexpr int tab_entries(unsigned width) { return tab_tag(width) + 1; }
static_assert(tab_entries(3) == 199, "the width-3 table");
constexpr int TAB_WORDS = 10;
constexpr size_t tab_bytes(unsigned width) { return (size_t)tab_entries(width) * TAB_WORDS * 4; }

constexpr unsigned MAX_DEPTH = 40;
constexpr int TAIL_MAX = 1024;       // nodes the one-workgroup tail kernel can take over: (T + T / 2) x 32 B of LDS = 48 KB
constexpr int TAIL_BLOCK = 256;
// knob defaults: ZL_TUNE_POSEIDON_CHUNK / _TAIL / _DEV_MIN (README).  TAIL and DEV_MIN rest on MEASUREMENTS (profiles/poseidon_bench.log): DEV_MIN is
// the smallest power of two from which the device won every repetition against the host path on both curves; for TAIL every value up to 256 lies inside the
// run-to-run spread on a 2^20-leaf build (a level is ~0.45 ms of dependent arithmetic, not launch overhead) and 256 is the largest one round of the workgroup covers.
constexpr int DEFAULT_CHUNK = 1 << 20, DEFAULT_TAIL = 256, DEFAULT_DEV_MIN = 64;
constexpr size_t STAGE_BUDGET = (size_t)256 << 20;  // bytes of ZL_SLOT_POSEIDON one staged chunk may take
constexpr size_t FLAG_BYTES = 256;                  // the flag word's corner of the slot

// what a hash records at an arity: x^2, x^4, x^5 of its 8 W + partial S-boxes less the constant one
constexpr size_t trace_per_hash(unsigned arity) { return 3 * (size_t)(spec(arity).full_rounds * spec(arity).width + spec(arity).partial_rounds - 1); }
static_assert(trace_per_hash(2) == 234 && trace_per_hash(3) == 258 && trace_per_hash(4) == 285 && trace_per_hash(5) == 309, "78, 86, 95, 103 recorded S-boxes");
// the chain circuit's assignment (zl_poseidon_chain_assignments): 1, h_k, x0, x1, then per link the records of its arity-2 hash
constexpr int TRACE_PER_LINK = (int)trace_per_hash(2);

// the membership circuit's assignment (zl_poseidon_merkle_assignments): 1, root, leaf, then per level sibling, index bit, left, right and the 234 records of
// H(left, right)
constexpr int MERKLE_PER_LEVEL = 4 + TRACE_PER_LINK;
constexpr size_t merkle_row_elems(unsigned depth) { return 3 + (size_t)MERKLE_PER_LEVEL * depth; }
static_assert(merkle_row_elems(1) == 241 && (merkle_row_elems(MAX_DEPTH) + MAX_DEPTH + 3) * 32 < STAGE_BUDGET, "a row and its inputs fit one staged chunk at every depth");

// the hash circuit's assignment at an arity (zl_poseidon_hash_assignments): 1, digest, the inputs, then the hash's records; and the leaf-membership circuit's
// (zl_poseidon_merkle_leaf_assignments): 1, root, the preimage, the leaf hash's records, then the levels of the membership circuit
constexpr size_t hash_row_elems(unsigned arity) { return 2 + arity + trace_per_hash(arity); }
constexpr size_t leaf_row_elems(unsigned arity, unsigned depth) { return hash_row_elems(arity) + (size_t)MERKLE_PER_LEVEL * depth; }
static_assert(hash_row_elems(2) == 4 + TRACE_PER_LINK, "at arity 2 the hash row is the row of a one-link chain");
static_assert((leaf_row_elems(MAX_ARITY, MAX_DEPTH) + MAX_ARITY + MAX_DEPTH + 2) * 32 < STAGE_BUDGET, "a row and its inputs fit one staged chunk at every arity and depth");

// the encryption circuit's assignment (zl_poseidon_encrypt_assignments), rate = W - 1: 1, tag, the N rate ciphertext elements, the H header elements, the K key
// elements, the N rate plaintext elements, then x^2, x^4, x^5 of the S = (F - 1 - Z) + (SB + N - 1) F recorded S-boxes: F = 8 W + partial per permutation, less
// lane 0 of round 0 and the Z = max(0, rate - K) rate lanes without a key element in the first one.  The limits are the cipher's, with K >= 1.
constexpr size_t MAX_DUPLEX_KEY = 64, MAX_DUPLEX_HEADER = 64, MAX_DUPLEX_BLOCKS = 1024;
constexpr bool encrypt_shape_ok(unsigned width, size_t K, size_t H, size_t N) {
    return width_ok(width) && K >= 1 && K <= MAX_DUPLEX_KEY && H <= MAX_DUPLEX_HEADER && N >= 1 && N <= MAX_DUPLEX_BLOCKS;
}
constexpr size_t sboxes_per_permutation(unsigned width) { return (size_t)spec_of_width(width).full_rounds * width + spec_of_width(width).partial_rounds; }
constexpr size_t encrypt_sboxes(unsigned width, size_t K, size_t H, size_t N) {
    return sboxes_per_permutation(width) - 1 - (K < width - 1 ? width - 1 - K : 0) + (K / (width - 1) + 1 + H / (width - 1) + 1 + N - 1) * sboxes_per_permutation(width);
}
constexpr size_t encrypt_row_elems(unsigned width, size_t K, size_t H, size_t N) { return 2 + 2 * N * (width - 1) + H + K + 3 * encrypt_sboxes(width, K, H, N); }
static_assert(encrypt_row_elems(3, 2, 0, 1) == 1 + 3 + 2 + 2 + 948 - 3 && encrypt_row_elems(6, 2, 0, 1) == 1 + 6 + 2 + 5 + 930 - 6, "(2, 0, 1): 948 and 930 constraints at widths 3 and 6");
static_assert(encrypt_row_elems(MAX_WIDTH, MAX_DUPLEX_KEY, MAX_DUPLEX_HEADER, MAX_DUPLEX_BLOCKS) < ((size_t)1 << 31) &&
                  (encrypt_row_elems(MAX_WIDTH, MAX_DUPLEX_KEY, MAX_DUPLEX_HEADER, MAX_DUPLEX_BLOCKS) + MAX_DUPLEX_KEY + MAX_DUPLEX_HEADER + 2 * MAX_DUPLEX_BLOCKS * (MAX_WIDTH - 1) + 1) * 32 <
                      STAGE_BUDGET,
              "the longest row fits 31 bits, and with its inputs and dense outputs one staged chunk");

constexpr bool geometry_ok(size_t n, unsigned depth) { return depth >= 1 && depth <= MAX_DEPTH && ((n >> depth) == 0 || n == ((size_t)1 << depth)); }
constexpr size_t level_size(size_t n, unsigned k) { return k >= 64 ? (n ? 1 : 0) : (n >> k) + ((n & (((size_t)1 << k) - 1)) ? 1 : 0); }  // ceil(n / 2^k)
constexpr size_t level_offset(size_t n, unsigned k) {  // elements in front of level k
    size_t off = 0;
    for (unsigned l = 0; l < k; l++) off += level_size(n, l);
    return off;
}
}  // namespace poseidon_dev
}  // namespace openzl

// The fused prover's producer (zl_groth16.hip): the assignments of `count` chains from HOST inputs straight into rows in DEVICE memory (row i at d_rows + i *
// stride_elems elements, 16-byte aligned), h_k of every chain to public_out (host, may be null).  Inputs are staged through ZL_SLOT_POSEIDON, launches are of at
// most ZL_TUNE_POSEIDON_CHUNK chains; finished on return, ZL_EINVAL for an input >= r.  ctx's device is current; curve and k are the caller's to check.
struct zl_ctx;
int zl_poseidon_trace_rows(zl_ctx* ctx, int curve, const uint64_t* x0, const uint64_t* x1, uint32_t k, size_t count, void* d_rows, size_t stride_elems, uint64_t* public_out);
// The membership producers of the fused prover, under the same rules.  _merkle_trace_rows: HOST leaves, indices and paths -> rows in DEVICE memory, the root of
// every fold to roots_out (host, may be null).  _merkle_member_rows: a node array in DEVICE memory (zl_poseidon_merkle_build_dev's layout) and HOST indices ->
// rows at d_rows (device), or, when host_rows is not null, dense rows staged on the device and downloaded to host_rows (d_rows and stride_elems are then unused).
// Curve, depth, n and the index bounds are the caller's to check.
int zl_poseidon_merkle_trace_rows(zl_ctx* ctx, int curve, const uint64_t* leaves, const uint64_t* indices, const uint64_t* paths, unsigned depth, size_t count, void* d_rows,
                                  size_t stride_elems, uint64_t* roots_out);
int zl_poseidon_merkle_member_rows(zl_ctx* ctx, int curve, const void* d_nodes, size_t n, unsigned depth, const uint64_t* indices, size_t count, void* d_rows,
                                   size_t stride_elems, uint64_t* host_rows);
// The producers of the arity-general provers (zl_groth16_prove_poseidon_hashes, zl_groth16_prove_merkle_leaf_paths / _members), under the same rules; arity
// (2..5) is the caller's to check too.  _hash_trace_rows: HOST inputs (count x arity) -> rows in DEVICE memory, the digests to public_out.  _merkle_leaf_trace_rows:
// HOST preimages (count x arity), indices and paths -> rows in DEVICE memory, the roots to roots_out.  _merkle_leaf_member_rows: a node array and the n x arity
// preimages of its leaves in DEVICE memory, HOST indices -> rows at d_rows, or staged and downloaded to host_rows when that is not null; ZL_EINVAL when a
// preimage does not hash to its leaf.
int zl_poseidon_hash_trace_rows(zl_ctx* ctx, int curve, unsigned arity, const uint64_t* in, size_t count, void* d_rows, size_t stride_elems, uint64_t* public_out);
int zl_poseidon_merkle_leaf_trace_rows(zl_ctx* ctx, int curve, unsigned arity, const uint64_t* preimages, const uint64_t* indices, const uint64_t* paths, unsigned depth,
                                       size_t count, void* d_rows, size_t stride_elems, uint64_t* roots_out);
int zl_poseidon_merkle_leaf_member_rows(zl_ctx* ctx, int curve, unsigned arity, const void* d_nodes, const void* d_preimages, size_t n, unsigned depth,
                                        const uint64_t* indices, size_t count, void* d_rows, size_t stride_elems, uint64_t* host_rows);
// The encryption producer of the fused prover (zl_groth16_prove_poseidon_encryptions), under the same rules: HOST keys (count x key_len), headers (count x
// header_len) and plaintexts (count x blocks x (width - 1)) -> rows in DEVICE memory; tags_out / ciphertexts_out (host, may be null) receive the tag and the
// ciphertext of every item.  Curve, width, the lengths and initial_state (NULL = zero, each element below r) are checked here as zl_poseidon_encrypt_assignments does.
int zl_poseidon_encrypt_trace_rows(zl_ctx* ctx, int curve, unsigned width, const uint64_t* initial_state, const uint64_t* keys, size_t key_len, const uint64_t* headers,
                                   size_t header_len, const uint64_t* plaintexts, size_t blocks, size_t count, void* d_rows, size_t stride_elems, uint64_t* tags_out,
                                   uint64_t* ciphertexts_out);
// The encryption trace inside ANOTHER circuit's rows (zl_circuit_hybrid_encrypt: the embedded-curve unit owns the row and its chunk).  Where the cipher's cells
// lie in such a row, in elements from the row's start: the tag, the N rate ciphertext elements, the H header elements, the N rate plaintext elements and the 3 S
// records are WRITTEN there; the key -- key_len elements, key_len >= 1 -- is READ from the row's own cells at `key` (some earlier launch on the stream wrote
// them) and not copied anywhere; [0] is not written.  zl_poseidon_encrypt_assignments' own row is the other layout of the same kernel body: key read from the
// call's keys and copied into cells, [0] = 1 written.
struct zl_duplex_row_layout {
    size_t tag, ct, header, key, plain, rec;
};
// _params: the cipher's validation (curve, width, lengths, initial_state -- NULL = zero, each element below r) -> init_out, 4 * MAX_WIDTH words.
// _launch: ONE launch of m rows on ctx's stream, no staging and no slot of this unit (the caller's chunk holds everything): row i at d_rows + i * stride_elems
// elements (16-byte aligned), headers and plaintexts dense in DEVICE memory, d_tags / d_cts (device, may be null) receive the tag and the ciphertext of every
// row, d_flag is the caller's flag word (bit 0 raised for a header, plaintext or key element >= r).  Not finished on return.  m is the caller's to bound.
// _host: the byte-identical host mirror over the host pool, rows, headers and plaintexts in HOST memory; ZL_EINVAL for an element >= r.
int zl_poseidon_duplex_row_params(int curve, unsigned width, const uint64_t* initial_state, size_t key_len, size_t header_len, size_t blocks, uint64_t* init_out);
int zl_poseidon_duplex_row_launch(zl_ctx* ctx, int curve, unsigned width, const uint64_t* init, const zl_duplex_row_layout& lay, size_t key_len, const void* d_headers,
                                  size_t header_len, const void* d_plaintexts, size_t blocks, size_t m, void* d_rows, size_t stride_elems, void* d_tags, void* d_cts,
                                  uint32_t* d_flag);
int zl_poseidon_duplex_row_host(int curve, unsigned width, const uint64_t* init, const zl_duplex_row_layout& lay, size_t key_len, const uint64_t* headers, size_t header_len,
                                const uint64_t* plaintexts, size_t blocks, size_t count, uint64_t* rows, size_t stride_elems);
// The forest producer of the fused prover (zl_groth16_prove_forest_members).  _prover_view: ZL_EINVAL for a null or host-mirror forest or a ctx of another
// device, else the forest's curve and depth.  _members_ok: ZL_EINVAL unless every (tree_of[i], indices[i]) names a leaf the forest holds.  _member_rows:
// zl_poseidon_merkle_member_rows with a tree per item, issued on ctx (the forest's own ctx or another lane of its device); roots_out (host, may be null)
// receives the root of every item.
struct zl_merkle_forest;
int zl_merkle_forest_prover_view(const zl_merkle_forest* f, const zl_ctx* ctx, int* curve, unsigned* depth);
int zl_merkle_forest_members_ok(const zl_merkle_forest* f, const uint32_t* tree_of, const uint64_t* indices, size_t count);
int zl_merkle_forest_member_rows(zl_ctx* ctx, const zl_merkle_forest* f, const uint32_t* tree_of, const uint64_t* indices, size_t count, void* d_rows, size_t stride_elems,
                                 uint64_t* host_rows, uint64_t* roots_out);
