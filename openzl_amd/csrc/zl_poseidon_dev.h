// zl_poseidon_dev.h -- internal layout and limits of the batched Poseidon unit (zl_poseidon_dev.hip): the device constant table, the knob defaults and the
// Merkle node-array geometry shared by the host path, the device path and the gather.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace openzl {
namespace poseidon_dev {
constexpr int WIDTH = 3, FULL_ROUNDS = 8, PARTIAL_ROUNDS = 55, ROUNDS = FULL_ROUNDS + PARTIAL_ROUNDS;
// the device table of one curve: entries of TAB_WORDS u32 slots holding the nine 29-bit limbs of x R' mod r (R' = 2^261: the device multiplier's own Montgomery form)
constexpr int TAB_KEYS = 0;                     // 189 round keys, [3 * round + lane]
constexpr int TAB_MDS = WIDTH * ROUNDS;         // 9 MDS entries, [3 * row + column]
constexpr int TAB_TAG = TAB_MDS + WIDTH * WIDTH;  // the arity-2 domain tag 3
constexpr int TAB_ENTRIES = TAB_TAG + 1;
constexpr int TAB_WORDS = 10;
constexpr size_t TAB_BYTES = (size_t)TAB_ENTRIES * TAB_WORDS * 4;

constexpr unsigned MAX_DEPTH = 40;
constexpr int TAIL_MAX = 1024;       // nodes the one-workgroup tail kernel can take over: (T + T / 2) x 32 B of LDS = 48 KB
constexpr int TAIL_BLOCK = 256;
// knob defaults: ZL_TUNE_POSEIDON_CHUNK / _TAIL / _DEV_MIN (README).  TAIL and DEV_MIN rest on MEASUREMENTS (profiles/poseidon_bench.log): DEV_MIN is
// the smallest power of two from which the device won every repetition against the host path on both curves; for TAIL every value up to 256 lies inside the
// run-to-run spread on a 2^20-leaf build (a level is ~0.45 ms of dependent arithmetic, not launch overhead) and 256 is the largest one round of the workgroup covers.
constexpr int DEFAULT_CHUNK = 1 << 20, DEFAULT_TAIL = 256, DEFAULT_DEV_MIN = 64;
constexpr size_t STAGE_BUDGET = (size_t)256 << 20;  // bytes of ZL_SLOT_POSEIDON one staged chunk may take
constexpr size_t FLAG_BYTES = 256;                  // the flag word's corner of the slot

// the chain circuit's assignment (zl_poseidon_chain_assignments): 1, h_k, x0, x1, then per link x^2, x^4, x^5 of its 79 S-boxes less the constant one
constexpr int TRACE_PER_LINK = 3 * (FULL_ROUNDS * WIDTH + PARTIAL_ROUNDS - 1);
static_assert(TRACE_PER_LINK == 234, "78 recorded S-boxes per link");

// the membership circuit's assignment (zl_poseidon_merkle_assignments): 1, root, leaf, then per level sibling, index bit, left, right and the 234 records of
// H(left, right)
constexpr int MERKLE_PER_LEVEL = 4 + TRACE_PER_LINK;
constexpr size_t merkle_row_elems(unsigned depth) { return 3 + (size_t)MERKLE_PER_LEVEL * depth; }
static_assert(merkle_row_elems(1) == 241 && (merkle_row_elems(MAX_DEPTH) + MAX_DEPTH + 3) * 32 < STAGE_BUDGET, "a row and its inputs fit one staged chunk at every depth");

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
