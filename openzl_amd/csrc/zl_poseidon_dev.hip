// zl_poseidon_dev.hip -- batched Poseidon on the device (include/zl_backend_ext.h): many permutations and hashes (widths 3..6), arity-2 hash
// chains and Merkle trees per call, one lane per permutation, with a host path (the host mirror's permute_native over the library's thread pool) behind the same
// entry points.  One unit for both scalar fields; built with the multiplier inlined (ZL_INLINE_MUL_DEVICE).  Every staged or chunked call goes through ONE
// runner, run_chunks (segments, upload, one launch per chunk, download, the flag read once); the width-3 entry points are the width-general ones at W = 3.
//
// Kernels (all templates over the scalar-field parameters FrP):
//   k_pos_chain / k_pos_fold / k_pos_level   one lane per chain / path / parent node (chain and fold: the dependent hashes in a loop inside the lane).  Thin
//                    wrappers around ONE __device__ width-3 permutation, permute_dev: the three state elements stay in registers for all 63 rounds; round
//                    keys, MDS entries and the domain tag come from a 199-entry device table (zl_poseidon_dev.h) at wave-uniform addresses -- the compiler
//                    reads them with uniform loads -- already in the multiplier's Montgomery form (x R', R' = 2^261).
//   k_pos_chain_trace  k_pos_chain that also WRITES what the lane computes on the way: the complete assignment of zl_circuit_poseidon_chain(curve, k, x0, x1)
//                    -- 1, h_k, x0, x1, then x^2, x^4, x^5 of every S-box the circuit allocates -- as one row of canonical words per chain.
//   k_pos_merkle_trace  k_pos_fold that writes the complete assignment of zl_circuit_poseidon_merkle(curve, depth, leaf, index, path) per path: 1, root, leaf,
//                    then per level the sibling, the index bit, the two selected hash inputs and the 234 records of the hash.  Templated over where the
//                    siblings come from: explicit paths, or the node array of a tree (membership of leaf `index`).
//   k_pos_tail       one workgroup finishes ALL remaining levels of a Merkle tree once a level has at most T nodes: the level lives in LDS (two buffers,
//                    canonical words), __syncthreads() between levels, every level is also written to the node array at the offsets the wide path uses.
//   k_pos_gather     sibling digests of `count` leaves out of a device node array.
//   k_pos_forest_place / _level / _gather   the Merkle forest (zl_merkle_forest_*): many growing trees in one allocation, each in the node layout of its capacity.
//                    An append places its leaves, then hashes per level the parents with a new leaf below them -- one lane each, ALL touched trees in one
//                    launch, the lane's tree found by binary search in the level's prefix sums; no one-workgroup tail.  ForestSrc lets k_pos_merkle_trace
//                    read memberships out of it.  With a null ctx the forest is its host mirror in host memory (host_forest_append).
//   k_pos_permute_w / k_pos_hash_w   the batched permutation and hash at every width of pd::spec (3..6: arity 2..5), one lane per permutation, through
//                    permute_any<FrP, W>: width 3 is permute_dev, widths 4, 5, 6 their own permutation permute_w<FrP, W> on W state registers and a table
//                    per (curve, width); there the S-box reduces its input weakly where the lazy bound requires it (the argument stands above WideBounds).
//   k_pos_hash_trace / k_pos_leaf_merkle_trace   the assignments of the arity-general circuits (zl_circuit_poseidon_hash / _merkle_leaf), widths 3..6, one lane per
//                    row: permute_w with a recorder writes the S-box records of the hash; the leaf-membership kernel then hands the digest -- reduced weakly
//                    (HandOver) -- to `depth` width-3 levels laid out as k_pos_merkle_trace's.  Sources: explicit preimages and paths, or a tree's node array beside
//                    its leaves' preimages, where a preimage that does not hash to its leaf raises a second flag bit.
//   k_pos_duplex     the duplex-sponge cipher (zl_poseidon_duplex_*), widths 3..6: one lane per message, its key, header and message blocks absorbed into the rate
//                    between the SB + N dependent permutations of ONE launch (permute_any); encrypt and decrypt are one template with a wave-uniform mode.  The
//                    absorbed lanes are outside the permutations' bound arguments and are reduced weakly at once (DuplexBounds).
//   k_pos_duplex_trace_in   k_pos_duplex_trace's body (duplex_trace_row) inside the rows of a circuit that holds the cipher: the cells where a row-layout
//                    descriptor says, the key read from the row itself (zl_circuit_hybrid_encrypt's agreed point), launched for the embedded-curve unit.
//   k_pos_duplex_trace   k_pos_duplex, encrypting, with the witness written out: the complete assignment of zl_circuit_poseidon_encrypt per message -- 1, tag,
//                    ciphertext, header, key, plaintext, then the records of the SB + N permutations -- under the circuit's round-0 record mask (rec0_mask): the
//                    first permutation drops lane 0 and the rate lanes without a key element, every later one records all of its S-boxes (DuplexTraceBounds).
// Arithmetic: the lazily reduced 9 x 29-bit Fr of zl_field28r.h (the NTT's multiplier), 1.29 - 1.46 x the carry-chain Fp<FrP> here and ahead of the 10 x 28 form at
// every size measured (profiles/poseidon_field_ab.log); the bound argument stands beside the type below.  The host path stays on Fp<FrP>.
// A lane at or above the item count returns before it reads or writes anything.  An input element >= r sets the flag word (atomicOr) and the lane goes on with
// the value as it is: the conversion product takes any 256-bit operand within its bound, the result is then meaningless and the call returns ZL_EINVAL.
#include <string.h>
#include <atomic>
#include <functional>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>
#include "zl_ctx.h"
#include "zl_host.h"
#include "zl_poseidon_dev.h"
#include "zl_field28r.h"

using namespace openzl;
namespace pd = openzl::poseidon_dev;

// The Merkle forest behind zl_merkle_forest_* (include/zl_backend_ext.h): `trees` node arrays of `stride` = zl_poseidon_merkle_nodes(capacity, depth) elements
// each in ONE allocation -- device memory of ctx's device, or host memory when ctx is null (the host mirror) -- and the trees' lengths, which live on the host.
struct zl_merkle_forest {
    zl_ctx* ctx = nullptr;
    zl_curve_t curve = ZL_BLS12_381;
    uint32_t trees = 0;
    unsigned depth = 0;
    size_t capacity = 0, stride = 0;
    uint64_t* nodes = nullptr;
    std::vector<uint64_t> lens;
    std::vector<uint64_t> add;  // an append's leaves per tree while it is planned; all zero between calls
};

namespace {
// ---------------------------------------------------------------------------------------------------------------- element I/O of the host path (Fp<FrP>)
// canonical u64 words -> Montgomery; false when the value is not below r
template <class FrP>
ZL_HD bool load_canon(const uint64_t* w, Fp<FrP>& out) {
    static_assert(FrP::N == 8, "scalar fields are 8 x 32 bits");
    Fp<FrP> c;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        c.l[2 * i] = (uint32_t)w[i];
        c.l[2 * i + 1] = (uint32_t)(w[i] >> 32);
    }
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) br = (((uint64_t)c.l[i] - FrP::mod(i) - br) >> 32) & 1;
    out = zl::to_mont(c);
    return br != 0;
}
template <class FrP>
ZL_HD void store_canon(uint64_t* w, const Fp<FrP>& m) {
    const Fp<FrP> c = zl::from_mont(m);
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = (uint64_t)c.l[2 * i] | ((uint64_t)c.l[2 * i + 1] << 32);
}


// ---------------------------------------------------------------------------------------------------------------- the device field: 9 x 29-bit lazy Fr
// zl_field28r.h's 9 x 29 instance (R' = 2^261), chosen by an interleaved A/B against the carry-chain Fp<FrP> and the 10 x 28 instance (profiles/poseidon_field_ab.log).
// Everything is kept as x R' in the multiplier's own Montgomery form and is only BOUNDED, never compared with r, until the final canon.  Bounds in units of r
// (the argument above k_test_poseidon28r, restated for these kernels):
//   * a product is < 2r; a loaded element is mul(c, R'^2) with c < 2^256 < 5.3 r (BN254; 2.3 r on BLS12-381) and R'^2 mod r < r: < 2r, canonical or not;
//   * a table entry (round key, MDS entry, tag) is < 2r; an MDS row is a sum of three products: < 6r;
//   * a state element entering a round is < 6r (from the MDS product, or the digest of the previous hash of a chain / fold / tree level) or < 2r (loaded);
//     plus its round key: < 8r.  S-box: x^2 = mul(x, x) needs 8 * 8 = 64, x^4 = mul(x^2, x^2) 2 * 2, x^5 = mul(x^4, x) 2 * 8; the MDS product multiplies an
//     entry < 2r by an element < 8r (the lanes a partial round leaves without S-box): 16.  The largest requirement, 64, is within MUL_BOUND of both fields
//     (70 and 169: the static_assert below);
//   * sums stay below 8r < 2^259: far inside the 261 bits of nine limbs and wred's limit of 128 r; the output is canon(mul(x, 1)): a product < 2r;
//   * the values k_pos_chain_trace records -- x^2, x^4, x^5 of an S-box -- are products themselves (< 2r), so dstore's mul(x, 1) takes them at 2 * 1 and
//     its canon sees a product again; recording reads the S-box's intermediates and changes none of them, so every bound above holds unchanged;
//   * k_pos_merkle_trace also records `left` and `right` of every level: each is a loaded element (the sibling, or the leaf at level 0: < 2r) or the digest of
//     the level below (element 0 of an MDS product: < 6r).  dstore's mul(x, 1) takes that at 6 * 1, far below 64, and hands canon a product (< 2r) as before;
//     the recorded copies are stored and the originals enter the permutation as in k_pos_fold, so no other bound changes.
template <class FrP> struct LazyP;
template <> struct LazyP<BLS12_381_Fr> { using P = BLS12_381_Fr29; };
template <> struct LazyP<BN254_Fr> { using P = BN254_Fr29; };
template <class FrP> using El = Fr28<typename LazyP<FrP>::P>;
static_assert(BLS12_381_Fr29::MUL_BOUND >= 64 && BN254_Fr29::MUL_BOUND >= 64, "x^2 of a state element < 8r needs B(a) B(b) = 64");
constexpr int TABW = pd::TAB_WORDS;  // u32 words per table entry (nine limbs used)
static_assert(El<BLS12_381_Fr>::L <= TABW && El<BN254_Fr>::L <= TABW, "a table entry holds every limb");
template <class FrP>
ZL_HD El<FrP> ezero() { El<FrP> r; for (int i = 0; i < El<FrP>::L; i++) r.l[i] = 0; return r; }
template <class FrP>
ZL_HD El<FrP> to_lazy(const uint32_t* c) {  // 8 x 32-bit words of a value < 2^256 -> x R' (< 2r)
    using P = typename LazyP<FrP>::P;
    uint32_t rp[8];
    for (int k = 0; k < 8; k++) rp[k] = P::rp2(k);
    return zl::mul(zl::unpack28r<P>(c), zl::unpack28r<P>(rp));
}
template <class FrP>
__device__ __forceinline__ bool dload(const uint64_t* w, El<FrP>& out) {
    uint32_t c[8];
#pragma unroll
    for (int i = 0; i < 4; i++) { c[2 * i] = (uint32_t)w[i]; c[2 * i + 1] = (uint32_t)(w[i] >> 32); }
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) br = (((uint64_t)c[i] - FrP::mod(i) - br) >> 32) & 1;
    out = to_lazy<FrP>(c);
    return br != 0;
}
template <class FrP>
__device__ __forceinline__ void dstore(uint64_t* w, const El<FrP>& m) {
    using P = typename LazyP<FrP>::P;
    uint32_t o[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    const El<FrP> c = zl::canon(zl::mul(m, zl::unpack28r<P>(o)));
    uint32_t v[8];
    zl::pack28r<P>(v, c);
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = (uint64_t)v[2 * i] | ((uint64_t)v[2 * i + 1] << 32);
}
// the same into a 16-byte aligned destination: two 16-byte stores instead of four 8-byte ones (the rows of k_pos_chain_trace)
template <class FrP>
__device__ __forceinline__ void dstore16(uint64_t* w, const El<FrP>& m) {
    using P = typename LazyP<FrP>::P;
    uint32_t o[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    const El<FrP> c = zl::canon(zl::mul(m, zl::unpack28r<P>(o)));
    uint32_t v[8];
    zl::pack28r<P>(v, c);
    ulonglong2* q = reinterpret_cast<ulonglong2*>(w);
    q[0] = make_ulonglong2((uint64_t)v[0] | ((uint64_t)v[1] << 32), (uint64_t)v[2] | ((uint64_t)v[3] << 32));
    q[1] = make_ulonglong2((uint64_t)v[4] | ((uint64_t)v[5] << 32), (uint64_t)v[6] | ((uint64_t)v[7] << 32));
}
// ---------------------------------------------------------------------------------------------------------------- the device permutation
// What an S-box hands to its recorder: nothing (every kernel but the trace), or x^2, x^4, x^5 appended to the lane's assignment row.
struct NoRec {
    template <class E>
    __device__ __forceinline__ void operator()(const E&, const E&, const E&) {}
};
template <class FrP>
struct RowRec {
    uint64_t* w;  // the next record of the lane's row
    __device__ __forceinline__ void operator()(const El<FrP>& x2, const El<FrP>& x4, const El<FrP>& x5) {
        dstore16<FrP>(w, x2);
        dstore16<FrP>(w + 4, x4);
        dstore16<FrP>(w + 8, x5);
        w += 12;
    }
};
template <class FrP>
__device__ __forceinline__ El<FrP> tab_ld(const uint32_t* __restrict__ tab, int entry) {
    El<FrP> r;
#pragma unroll
    for (int k = 0; k < El<FrP>::L; k++) r.l[k] = tab[entry * TABW + k];
    return r;
}
template <class FrP, class Rec>
__device__ __forceinline__ void sbox(El<FrP>& x, Rec& rec, bool recorded) {
    const El<FrP> x2 = zl::mul(x, x), x4 = zl::mul(x2, x2);
    x = zl::mul(x4, x);
    if (recorded) rec(x2, x4, x);
}
// 63 rounds of add-round-key / x^5 / MDS: 8 * (9 + 9) + 55 * (3 + 9) = 804 multiplications.  One rolled loop (18 inlined multiplier bodies), the full / partial
// choice is a wave-uniform branch.  `rec` sees the S-boxes in the order the in-circuit hash allocates them, without lane 0 of round 0: its input is the domain
// tag plus a round key, a constant, and the circuit folds it (poseidon::hash in zl_host.h; permute_native_record is the host's form of this).
// skip0 is that rule as a mask: bit i set = lane i of round 0 is NOT recorded.  Every caller but k_pos_duplex_trace leaves it at the compile-time default, lane 0
// alone, which folds to the `rnd != 0` / `true` the S-boxes were written with; the encryption circuit folds more lanes of its first permutation and none of
// the later ones (rec0_mask).
constexpr uint32_t SKIP0_HASH = 1u;
__device__ __forceinline__ bool rec_lane(int rnd, uint32_t skip0, int lane) { return rnd != 0 || !((skip0 >> lane) & 1u); }
template <class FrP, class Rec>
__device__ __forceinline__ void permute_dev(const uint32_t* __restrict__ tab, El<FrP>& s0, El<FrP>& s1, El<FrP>& s2, Rec& rec, const uint32_t skip0 = SKIP0_HASH) {
    constexpr pd::Spec S = pd::spec(2);
    constexpr int half = (int)S.full_rounds / 2, partial = (int)S.partial_rounds, rounds = (int)S.rounds();
#pragma unroll 1
    for (int rnd = 0; rnd < rounds; rnd++) {
        s0 = zl::add(s0, tab_ld<FrP>(tab, pd::tab_keys(3) + 3 * rnd));
        s1 = zl::add(s1, tab_ld<FrP>(tab, pd::tab_keys(3) + 3 * rnd + 1));
        s2 = zl::add(s2, tab_ld<FrP>(tab, pd::tab_keys(3) + 3 * rnd + 2));
        sbox<FrP>(s0, rec, rec_lane(rnd, skip0, 0));
        if (rnd < half || rnd >= half + partial) {
            sbox<FrP>(s1, rec, rec_lane(rnd, skip0, 1));
            sbox<FrP>(s2, rec, rec_lane(rnd, skip0, 2));
        }
        El<FrP> nx[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            El<FrP> acc = zl::mul(tab_ld<FrP>(tab, pd::tab_mds(3) + 3 * i), s0);
            acc = zl::add(acc, zl::mul(tab_ld<FrP>(tab, pd::tab_mds(3) + 3 * i + 1), s1));
            nx[i] = zl::add(acc, zl::mul(tab_ld<FrP>(tab, pd::tab_mds(3) + 3 * i + 2), s2));
        }
        s0 = nx[0];
        s1 = nx[1];
        s2 = nx[2];
    }
}
// H(x, y) on Montgomery operands
template <class FrP>
__device__ __forceinline__ El<FrP> hash2_dev(const uint32_t* __restrict__ tab, const El<FrP>& x, const El<FrP>& y) {
    El<FrP> s0 = tab_ld<FrP>(tab, pd::tab_tag(3)), s1 = x, s2 = y;
    NoRec none;
    permute_dev<FrP>(tab, s0, s1, s2, none);
    return s0;
}

// ---------------------------------------------------------------------------------------------------------------- kernels
constexpr int BLOCK = 64;

template <class FrP>
__global__ __launch_bounds__(BLOCK) void k_pos_chain(const uint32_t* __restrict__ tab, const uint64_t* __restrict__ x0, const uint64_t* __restrict__ x1, uint32_t k,
                                                     size_t n, uint64_t* __restrict__ out, uint32_t* __restrict__ flag) {
    const size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    El<FrP> h, b;
    bool ok = dload<FrP>(x0 + p * 4, h);
    ok &= dload<FrP>(x1 + p * 4, b);
    if (!ok) atomicOr(flag, 1u);
#pragma unroll 1
    for (uint32_t j = 0; j < k; j++) h = hash2_dev<FrP>(tab, h, b);
    dstore<FrP>(out + p * 4, h);
}
// k_pos_chain with the witness written out: row p = out + p * stride elements (16-byte aligned) receives [0] = 1, [1] = h_k, [2] = x0, [3] = x1 and, from [4] on,
// the 234 records of each link in turn; elements from 4 + 234 k to the stride are not touched.  pub (may be null) receives h_k once more, densely.  Every lane
// stores 32 bytes at a time at a stride of one row.  Measured against rows staged through LDS (a wave then writes runs of 288 bytes): 12 - 15 % ahead from 2^10
// to 2^16 chains, where a launch takes the 0.56 ms of ONE chain whatever its width, 13 % behind at 2^18 (profiles/chain_trace_layout_ab.log);
// the batched prover's chunks stay below 2^13 chains.
template <class FrP>
__global__ __launch_bounds__(BLOCK) void k_pos_chain_trace(const uint32_t* __restrict__ tab, const uint64_t* __restrict__ x0, const uint64_t* __restrict__ x1, uint32_t k,
                                                           size_t n, uint64_t* __restrict__ out, size_t stride, uint64_t* __restrict__ pub, uint32_t* __restrict__ flag) {
    const size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    El<FrP> h, b;
    bool ok = dload<FrP>(x0 + p * 4, h);
    ok &= dload<FrP>(x1 + p * 4, b);
    if (!ok) atomicOr(flag, 1u);
    uint64_t* row = out + p * stride * 4;
    RowRec<FrP> rec{row + 16};
#pragma unroll 1
    for (uint32_t j = 0; j < k; j++) {
        El<FrP> s0 = tab_ld<FrP>(tab, pd::tab_tag(3)), s2 = b;
        permute_dev<FrP>(tab, s0, h, s2, rec);
        h = s0;
    }
    ulonglong2* q = reinterpret_cast<ulonglong2*>(row);
    q[0] = make_ulonglong2(1, 0);
    q[1] = make_ulonglong2(0, 0);
    dstore16<FrP>(row + 4, h);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        row[8 + i] = x0[p * 4 + i];
        row[12 + i] = x1[p * 4 + i];
    }
    if (pub) dstore<FrP>(pub + p * 4, h);
}
// one lane per path: `depth` dependent hashes, the running digest on the right when the index bit of the level is set
template <class FrP>
__global__ __launch_bounds__(BLOCK) void k_pos_fold(const uint32_t* __restrict__ tab, const uint64_t* __restrict__ leaves, const uint64_t* __restrict__ indices,
                                                    const uint64_t* __restrict__ paths, unsigned depth, size_t n, uint64_t* __restrict__ roots,
                                                    uint32_t* __restrict__ flag) {
    const size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    El<FrP> cur;
    bool ok = dload<FrP>(leaves + p * 4, cur);
    const uint64_t idx = indices[p];
    const uint64_t* path = paths + p * (size_t)depth * 4;
#pragma unroll 1
    for (unsigned k = 0; k < depth; k++) {
        El<FrP> sib;
        ok &= dload<FrP>(path + (size_t)k * 4, sib);
        const bool right = (idx >> k) & 1;
        El<FrP> x, y;
#pragma unroll
        for (int w = 0; w < El<FrP>::L; w++) {
            x.l[w] = right ? sib.l[w] : cur.l[w];
            y.l[w] = right ? cur.l[w] : sib.l[w];
        }
        cur = hash2_dev<FrP>(tab, x, y);
    }
    if (!ok) atomicOr(flag, 1u);
    dstore<FrP>(roots + p * 4, cur);
}
// one Merkle level, wide: parent j of [first, first + n) = H(child 2j, child 2j + 1 or zero)
template <class FrP>
__global__ __launch_bounds__(BLOCK) void k_pos_level(const uint32_t* __restrict__ tab, const uint64_t* __restrict__ child, size_t n_child, uint64_t* __restrict__ parent,
                                                     size_t first, size_t n, uint32_t* __restrict__ flag) {
    const size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const size_t j = first + p;
    El<FrP> x, y = ezero<FrP>();
    bool ok = dload<FrP>(child + 2 * j * 4, x);
    if (2 * j + 1 < n_child) ok &= dload<FrP>(child + (2 * j + 1) * 4, y);
    if (!ok) atomicOr(flag, 1u);
    dstore<FrP>(parent + j * 4, hash2_dev<FrP>(tab, x, y));
}
// one workgroup, every level above `level` (m <= TAIL_MAX nodes at `level`, which starts the node range this kernel owns): LDS buffer A holds m nodes, B the
// ceil(m / 2) parents; the buffers swap per level.  Level l + 1 goes to level + off, off = the nodes of the levels in front of it, as in the wide path.
template <class FrP>
__global__ __launch_bounds__(pd::TAIL_BLOCK) void k_pos_tail(const uint32_t* __restrict__ tab, uint64_t* __restrict__ level, unsigned m, unsigned levels,
                                                             uint32_t* __restrict__ flag) {
    extern __shared__ uint64_t lds[];
    uint64_t* cur = lds;
    uint64_t* nxt = lds + (size_t)m * 4;
    for (unsigned i = threadIdx.x; i < m * 4; i += pd::TAIL_BLOCK) cur[i] = level[i];
    size_t off = m;
    unsigned cm = m;
    for (unsigned l = 0; l < levels; l++) {
        const unsigned pm = (cm + 1) / 2;
        __syncthreads();
        for (unsigned j = threadIdx.x; j < pm; j += pd::TAIL_BLOCK) {
            El<FrP> x, y = ezero<FrP>();
            bool ok = dload<FrP>(cur + 2 * j * 4, x);
            if (2 * j + 1 < cm) ok &= dload<FrP>(cur + (2 * j + 1) * 4, y);
            if (!ok) atomicOr(flag, 1u);
            uint64_t w[4];
            dstore<FrP>(w, hash2_dev<FrP>(tab, x, y));
#pragma unroll
            for (int i = 0; i < 4; i++) {
                nxt[j * 4 + i] = w[i];
                level[(off + j) * 4 + i] = w[i];
            }
        }
        off += pm;
        cm = pm;
        uint64_t* t = cur;
        cur = nxt;
        nxt = t;
    }
}
struct LevelTable {
    uint64_t off[pd::MAX_DEPTH], size[pd::MAX_DEPTH];  // of levels 0 .. depth - 1: where a leaf's siblings live
};
// thread t = path t / depth, level t % depth: the sibling of (index >> level), zero where the tree has no such node
__global__ __launch_bounds__(BLOCK) void k_pos_gather(const uint64_t* __restrict__ nodes, LevelTable lt, unsigned depth, const uint64_t* __restrict__ indices, size_t total,
                                                      uint64_t* __restrict__ paths) {
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= total) return;
    const size_t p = t / depth;
    const unsigned k = (unsigned)(t % depth);
    const uint64_t sib = (indices[p] >> k) ^ 1;
    const bool present = sib < lt.size[k];
#pragma unroll
    for (int i = 0; i < 4; i++) paths[t * 4 + i] = present ? nodes[(lt.off[k] + sib) * 4 + i] : 0;
}
// Where k_pos_merkle_trace reads item p's leaf and its sibling at level k (nullptr: the tree has no such node, the sibling is the zero digest): explicit arrays
// of one leaf and `depth` siblings per item, or the node array of a tree (zl_poseidon_merkle_build_dev's layout) addressed by the item's leaf index.
struct PathSrc {
    const uint64_t* leaves;
    const uint64_t* paths;
    unsigned depth;
    __device__ __forceinline__ const uint64_t* leaf(size_t p, uint64_t) const { return leaves + p * 4; }
    __device__ __forceinline__ const uint64_t* sibling(size_t p, uint64_t, unsigned k) const { return paths + (p * depth + k) * 4; }
    PathSrc advanced(size_t first) const { return PathSrc{leaves + first * 4, paths + first * depth * 4, depth}; }  // the source of items first, first + 1, ...
};
struct TreeSrc {
    const uint64_t* nodes;
    LevelTable lt;
    __device__ __forceinline__ const uint64_t* leaf(size_t, uint64_t idx) const { return nodes + idx * 4; }
    __device__ __forceinline__ const uint64_t* sibling(size_t, uint64_t idx, unsigned k) const {
        const uint64_t sib = (idx >> k) ^ 1;
        return sib < lt.size[k] ? nodes + (lt.off[k] + sib) * 4 : nullptr;
    }
    TreeSrc advanced(size_t) const { return *this; }
};
// ... or one tree per item out of a Merkle forest: tree tree_of[p] starts `stride` elements after its predecessor and has the layout of the forest's CAPACITY
// (lt), whatever its length; a node that no leaf lies under is stored as zero there, which is what an absent sibling reads as.
struct ForestSrc {
    const uint64_t* nodes;
    size_t stride;
    const uint32_t* tree_of;  // device memory, one entry per item of the launch
    LevelTable lt;
    __device__ __forceinline__ const uint64_t* leaf(size_t p, uint64_t idx) const { return nodes + ((size_t)tree_of[p] * stride + idx) * 4; }
    __device__ __forceinline__ const uint64_t* sibling(size_t p, uint64_t idx, unsigned k) const {
        const uint64_t sib = (idx >> k) ^ 1;
        return sib < lt.size[k] ? nodes + ((size_t)tree_of[p] * stride + lt.off[k] + sib) * 4 : nullptr;
    }
    ForestSrc advanced(size_t) const { return *this; }  // (tree_of is staged per chunk: merkle_trace_run)
};
__device__ __forceinline__ void copy16(uint64_t* dst16, uint64_t a, uint64_t b, uint64_t c, uint64_t d) {  // one element of canonical words, dst 16-byte aligned
    ulonglong2* q = reinterpret_cast<ulonglong2*>(dst16);
    q[0] = make_ulonglong2(a, b);
    q[1] = make_ulonglong2(c, d);
}
// k_pos_fold with the witness written out: the complete assignment of zl_circuit_poseidon_merkle(curve, depth, leaf, index, path) per item, one lane each.
// Row p = out + p * stride elements (16-byte aligned): [0] = 1, [1] = root, [2] = leaf, then per level j at 3 + 238 j: [+0] the sibling, [+1] the index bit,
// [+2] left, [+3] right, [+4 .. +238) the 234 records of H(left, right); elements from 3 + 238 depth to the stride are not touched.  The lane writes its row
// front to back (the root last).  The select copies limbs as k_pos_fold does; left and right go out through dstore16 -- one of them is the loaded sibling
// (< 2r), the other the running digest (< 6r, or the loaded leaf): within mul(x, 1)'s bound, see above LazyP.  pub (may be null) receives the root, densely.
template <class FrP, class Src>
__global__ __launch_bounds__(BLOCK) void k_pos_merkle_trace(const uint32_t* __restrict__ tab, const Src src, const uint64_t* __restrict__ indices, unsigned depth, size_t n,
                                                            uint64_t* __restrict__ out, size_t stride, uint64_t* __restrict__ pub, uint32_t* __restrict__ flag) {
    const size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint64_t idx = indices[p];
    uint64_t* row = out + p * stride * 4;
    El<FrP> cur;
    const uint64_t* lw = src.leaf(p, idx);
    bool ok = dload<FrP>(lw, cur);
    copy16(row + 8, lw[0], lw[1], lw[2], lw[3]);
    uint64_t* lv = row + 12;
#pragma unroll 1
    for (unsigned k = 0; k < depth; k++) {
        const uint64_t* sw = src.sibling(p, idx, k);
        El<FrP> sib = ezero<FrP>();
        if (sw) {
            ok &= dload<FrP>(sw, sib);
            copy16(lv, sw[0], sw[1], sw[2], sw[3]);
        } else {
            copy16(lv, 0, 0, 0, 0);
        }
        const bool right = (idx >> k) & 1;
        copy16(lv + 4, right ? 1 : 0, 0, 0, 0);
        El<FrP> s0 = tab_ld<FrP>(tab, pd::tab_tag(3)), x, y;
#pragma unroll
        for (int w = 0; w < El<FrP>::L; w++) {
            x.l[w] = right ? sib.l[w] : cur.l[w];
            y.l[w] = right ? cur.l[w] : sib.l[w];
        }
        dstore16<FrP>(lv + 8, x);
        dstore16<FrP>(lv + 12, y);
        RowRec<FrP> rec{lv + 16};
        permute_dev<FrP>(tab, s0, x, y, rec);
        cur = s0;
        lv += (size_t)pd::MERKLE_PER_LEVEL * 4;
    }
    if (!ok) atomicOr(flag, 1u);
    copy16(row, 1, 0, 0, 0);
    dstore16<FrP>(row + 4, cur);
    if (pub) dstore<FrP>(pub + p * 4, cur);
}

// ---------------------------------------------------------------------------------------------------------------- the Merkle forest (zl_merkle_forest_*)
// `trees` trees side by side in one allocation, tree t at t * stride elements in the layout of zl_poseidon_merkle_build_dev for n = capacity; zero-filled at
// creation and written only where a leaf lies below.  An append places its leaves, then hashes level after level the parents that have a new leaf under them:
// ONE launch per level over all touched trees (split only at the launch chunk), never a one-workgroup tail -- a level costs one permutation latency whichever
// way it is launched, so the trees of a batch share each level's latency instead of queueing behind each other.
template <class FrP>
ZL_HD bool canon_words(const uint64_t* w) {  // the value of four u64 words is below r
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) br = (((uint64_t)(uint32_t)(w[i / 2] >> (32 * (i & 1))) - FrP::mod(i) - br) >> 32) & 1;
    return br != 0;
}
// one lane per new leaf: refuse it when it is not below r (the flag word; nothing is stored), else store it at element dst[p] of the allocation -- level 0 of
// its tree, the slot the host computed.  nodes == nullptr: check only (the validation pass of zl_merkle_forest_append_dev; dst is not read).
template <class FrP>
__global__ __launch_bounds__(BLOCK) void k_pos_forest_place(const uint64_t* __restrict__ leaves, const uint64_t* __restrict__ dst, size_t n, uint64_t* __restrict__ nodes,
                                                            uint32_t* __restrict__ flag) {
    const size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    uint64_t w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = leaves[p * 4 + i];
    if (!canon_words<FrP>(w)) {
        atomicOr(flag, 1u);
        return;
    }
    if (!nodes) return;
    uint64_t* at = nodes + dst[p] * 4;
#pragma unroll
    for (int i = 0; i < 4; i++) at[i] = w[i];
}
// The trees an append touches: tree[s] grew from first[s] to some larger length, so at level k it has the dirty parents first[s] >> k .. (last leaf) >> k, and
// pre[s] of them lie in the segments in front of s (pre has count + 1 entries, strictly increasing; pre[count] = the level's total).  All device memory.
struct ForestSegs {
    const uint32_t* tree;
    const uint64_t* first;
    const uint64_t* pre;  // the row of the launch's level
    uint32_t count;
};
// the segment of dirty parent q: the largest s with pre[s] <= q (q < pre[count]); at most 17 steps for 65 536 trees
ZL_HD uint32_t forest_seg(const uint64_t* pre, uint32_t count, uint64_t q) {
    uint32_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pre[mid] <= q) lo = mid;
        else hi = mid;
    }
    return lo;
}
// one lane per dirty parent of level k, over every touched tree: parent j = H(child 2j, child 2j + 1 -- zero beyond the capacity's level k - 1).  Lane p of the
// launch is dirty parent first + p of the level.  child_off / parent_off: the elements in front of levels k - 1 and k inside a tree.
template <class FrP>
__global__ __launch_bounds__(BLOCK) void k_pos_forest_level(const uint32_t* __restrict__ tab, uint64_t* nodes, size_t stride, const ForestSegs sg, unsigned k, size_t child_off,
                                                            size_t child_size, size_t parent_off, size_t first, size_t n, uint32_t* __restrict__ flag) {
    const size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint64_t q = first + p;
    const uint32_t s = forest_seg(sg.pre, sg.count, q);
    const size_t j = (size_t)(sg.first[s] >> k) + (size_t)(q - sg.pre[s]);
    uint64_t* tree = nodes + (size_t)sg.tree[s] * stride * 4;
    const uint64_t* left = tree + (child_off + 2 * j) * 4;
    uint64_t* parent = tree + (parent_off + j) * 4;
    El<FrP> x, y = ezero<FrP>();
    bool ok = dload<FrP>(left, x);
    if (2 * j + 1 < child_size) ok &= dload<FrP>(left + 4, y);
    if (!ok) atomicOr(flag, 1u);
    dstore<FrP>(parent, hash2_dev<FrP>(tab, x, y));
}
// k_pos_gather with a tree per item: thread t = item t / depth, level t % depth
__global__ __launch_bounds__(BLOCK) void k_pos_forest_gather(const uint64_t* __restrict__ nodes, size_t stride, LevelTable lt, unsigned depth, const uint32_t* __restrict__ tree_of,
                                                             const uint64_t* __restrict__ indices, size_t total, uint64_t* __restrict__ paths) {
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= total) return;
    const size_t p = t / depth;
    const unsigned k = (unsigned)(t % depth);
    const uint64_t sib = (indices[p] >> k) ^ 1;
    const bool present = sib < lt.size[k];
    const uint64_t* tree = nodes + (size_t)tree_of[p] * stride * 4;
#pragma unroll
    for (int i = 0; i < 4; i++) paths[t * 4 + i] = present ? tree[(lt.off[k] + sib) * 4 + i] : 0;
}

// ---------------------------------------------------------------------------------------------------------------- widths 4, 5, 6 (arity 3, 4, 5)
// The same schedule on W state elements (pd::spec: 8 + 55 rounds at width 4, 8 + 56 at widths 5 and 6), one lane per permutation, the state in registers, the
// constants from the table of the (curve, width) at wave-uniform addresses.  The width-3 bound argument (above LazyP) does NOT carry over; restated in units of r:
//   * a product, a loaded element and a table entry are < 2r as before; an MDS row is a sum of W products: < 2W r (8, 10, 12); a state element entering a
//     round is that or a loaded element / the tag (< 2r); plus its round key: < (2W + 2) r = KEYED r (10, 12, 14);
//   * squaring a keyed element would need KEYED^2 = 100, 144, 196: above MUL_BOUND = 70 of BLS12-381 at every width, above 169 of BN254 at width 6.  Exactly
//     there (REDUCE) the S-box first reduces its input weakly: wred takes a carried value below 128 r (add carries; KEYED <= 14) and returns < 2r, so x^2
//     needs 2 * 2, x^4 2 * 2, x^5 = mul(x^4, x) 2 * 2.  BN254 at widths 4 and 5 keeps the plain S-box: x^2 needs 100 resp. 144 <= 169, x^5 2 * KEYED.
//     One wred per S-box, 8 W + partial rounds per permutation, is the least that the arithmetic allows: every S-box input is a fresh row sum plus a key;
//   * the lanes a partial round leaves without S-box stay < KEYED r and enter the MDS product against an entry < 2r: 2 * KEYED = 20, 24, 28, fine everywhere,
//     so they are NOT reduced; the S-boxed lanes enter it at 2 * 2;
//   * the outputs are row sums (< 2W r): dstore's mul(x, 1) takes them at 2W * 1 and hands canon a product (< 2r);
//   * sums stay below 14 r < 2^259: inside nine limbs.
// WideBounds states this per (field, width) and asserts the largest bound product that reaches mul.
constexpr int cmax(int a, int b) { return a > b ? a : b; }
template <class FrP, int W>
struct WideBounds {
    using P = typename LazyP<FrP>::P;
    static constexpr int ROW = 2 * W;                                // an MDS row sum
    static constexpr int KEYED = ROW + 2;                            // ... plus a round key
    static constexpr bool REDUCE = KEYED * KEYED > P::MUL_BOUND;     // the S-box reduces its input first
    static constexpr int SBOX_IN = REDUCE ? 2 : KEYED;
    static constexpr int SBOX_MUL = cmax(SBOX_IN * SBOX_IN, cmax(2 * 2, 2 * SBOX_IN));  // x^2, x^4, x^5
    static constexpr int MDS_MUL = 2 * KEYED;                        // entry x a lane without S-box
    static constexpr int STORE_MUL = ROW * 1;                        // dstore: mul(x, 1), then canon of a product (< 2r, wred's limit is 128 r)
    static constexpr int MAX_MUL = cmax(SBOX_MUL, cmax(MDS_MUL, STORE_MUL));
    static_assert(MAX_MUL <= P::MUL_BOUND, "a bound product above what mul takes: place a weak reduction");
    static_assert(KEYED <= 128, "wred (and canon) take a value below 128 r");
};
#define ZL_POS_W_BOUNDS(FrP, W, reduce, max_mul) \
    static_assert(WideBounds<FrP, W>::REDUCE == reduce && WideBounds<FrP, W>::MAX_MUL == max_mul && WideBounds<FrP, W>::MAX_MUL <= LazyP<FrP>::P::MUL_BOUND, "bounds of " #FrP " at width " #W)
ZL_POS_W_BOUNDS(BLS12_381_Fr, 4, true, 20);   // keyed 10: 100 > 70, reduced; the largest product is the MDS's 2 * 10
ZL_POS_W_BOUNDS(BLS12_381_Fr, 5, true, 24);   // keyed 12: 144 > 70
ZL_POS_W_BOUNDS(BLS12_381_Fr, 6, true, 28);   // keyed 14: 196 > 70
ZL_POS_W_BOUNDS(BN254_Fr, 4, false, 100);     // 100 <= 169: no reduction
ZL_POS_W_BOUNDS(BN254_Fr, 5, false, 144);     // 144 <= 169: no reduction
ZL_POS_W_BOUNDS(BN254_Fr, 6, true, 28);       // 196 > 169, reduced
#undef ZL_POS_W_BOUNDS
static_assert(!WideBounds<BLS12_381_Fr, 3>::REDUCE && !WideBounds<BN254_Fr, 3>::REDUCE && WideBounds<BLS12_381_Fr, 3>::MAX_MUL == 64,
              "the same rule gives the width-3 unit's argument: no reduction, 64");

// With REDUCE the recorder sees x^2, x^4, x^5 of the reduced input: the same field element, and all three are products (< 2r) whichever way the input came.
template <class FrP, int W, class Rec>
__device__ __forceinline__ void sbox_w(El<FrP>& x, Rec& rec, bool recorded) {
    if constexpr (WideBounds<FrP, W>::REDUCE) x = zl::wred(x);
    const El<FrP> x2 = zl::mul(x, x), x4 = zl::mul(x2, x2);
    x = zl::mul(x4, x);
    if (recorded) rec(x2, x4, x);
}
// the S-boxes of lanes I .. W - 1 of a full round, one after the other.  A compile-time recursion, not a loop: with a recorder the body holds six multiplier
// bodies per lane, and at width 6 the loop unroller gives up on it -- the state would then be indexed at run time and leave its registers.
template <class FrP, int W, int I, class Rec>
__device__ __forceinline__ void sbox_lanes(El<FrP> (&s)[W], Rec& rec, int rnd, const uint32_t skip0) {
    if constexpr (I < W) {
        sbox_w<FrP, W>(s[I], rec, rec_lane(rnd, skip0, I));
        sbox_lanes<FrP, W, I + 1>(s, rec, rnd, skip0);
    }
}
// 8 (3W + W^2) + partial (3 + W^2) multiplications: 1 288, 1 976, 2 616 at widths 4, 5, 6.  One rolled round loop; the ROWS of the MDS product are a rolled loop
// too, so a round holds 3W + W inlined multiplier bodies instead of 3W + W^2 (24 instead of 54 at width 6): row i is accumulated against the W state registers
// and shifted into nx from the top, all register indices static, and after W rows nx[k] is row k.  Table addresses depend on the round and the row only.
// `rec` (NoRec, or RowRec in the trace kernels) sees the S-boxes in round order, lane order within a round, without lane 0 of round 0 -- the order in which
// poseidon::hash<FrP, W> of zl_host.h allocates them, as permute_dev's recorder does at width 3; skip0 as there.
template <class FrP, int W, class Rec>
__device__ __forceinline__ void permute_w(const uint32_t* __restrict__ tab, El<FrP> (&s)[W], Rec& rec, const uint32_t skip0 = SKIP0_HASH) {
    constexpr pd::Spec S = pd::spec_of_width(W);
    constexpr int half = (int)S.full_rounds / 2, partial = (int)S.partial_rounds, rounds = (int)S.rounds();
#pragma unroll 1
    for (int rnd = 0; rnd < rounds; rnd++) {
#pragma unroll
        for (int i = 0; i < W; i++) s[i] = zl::add(s[i], tab_ld<FrP>(tab, pd::tab_keys(W) + W * rnd + i));
        sbox_w<FrP, W>(s[0], rec, rec_lane(rnd, skip0, 0));
        if (rnd < half || rnd >= half + partial) sbox_lanes<FrP, W, 1>(s, rec, rnd, skip0);
        El<FrP> nx[W];
#pragma unroll
        for (int i = 0; i < W; i++) nx[i] = ezero<FrP>();
#pragma unroll 1
        for (int i = 0; i < W; i++) {
            El<FrP> acc = zl::mul(tab_ld<FrP>(tab, pd::tab_mds(W) + W * i), s[0]);
#pragma unroll
            for (int j = 1; j < W; j++) acc = zl::add(acc, zl::mul(tab_ld<FrP>(tab, pd::tab_mds(W) + W * i + j), s[j]));
#pragma unroll
            for (int k = 0; k + 1 < W; k++) nx[k] = nx[k + 1];
            nx[W - 1] = acc;
        }
#pragma unroll
        for (int i = 0; i < W; i++) s[i] = nx[i];
    }
}
// the permutation of any width of the table: width 3 is the width-3 unit's own permute_dev (what k_pos_chain_trace and k_pos_merkle_trace run), the wider
// ones permute_w
template <class FrP, int W, class Rec>
__device__ __forceinline__ void permute_any(const uint32_t* __restrict__ tab, El<FrP> (&s)[W], Rec& rec, const uint32_t skip0 = SKIP0_HASH) {
    if constexpr (W == 3) permute_dev<FrP>(tab, s[0], s[1], s[2], rec, skip0);
    else permute_w<FrP, W>(tab, s, rec, skip0);
}
// count x W elements, in place
template <class FrP, int W>
__global__ __launch_bounds__(BLOCK) void k_pos_permute_w(const uint32_t* __restrict__ tab, uint64_t* __restrict__ states, size_t n, uint32_t* __restrict__ flag) {
    const size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    uint64_t* st = states + p * (4 * W);
    El<FrP> s[W];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < W; i++) ok &= dload<FrP>(st + 4 * i, s[i]);
    if (!ok) atomicOr(flag, 1u);
    NoRec none;
    permute_any<FrP, W>(tab, s, none);
#pragma unroll
    for (int i = 0; i < W; i++) dstore<FrP>(st + 4 * i, s[i]);
}
// out[p] = element 0 of permute([tag, in[p][0], .., in[p][W - 2]]): the hash of W - 1 inputs
template <class FrP, int W>
__global__ __launch_bounds__(BLOCK) void k_pos_hash_w(const uint32_t* __restrict__ tab, const uint64_t* __restrict__ in, size_t n, uint64_t* __restrict__ out,
                                                      uint32_t* __restrict__ flag) {
    const size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint64_t* x = in + p * (4 * (W - 1));
    El<FrP> s[W];
    s[0] = tab_ld<FrP>(tab, pd::tab_tag(W));
    bool ok = true;
#pragma unroll
    for (int i = 1; i < W; i++) ok &= dload<FrP>(x + 4 * (i - 1), s[i]);
    if (!ok) atomicOr(flag, 1u);
    NoRec none;
    permute_any<FrP, W>(tab, s, none);
    dstore<FrP>(out + p * 4, s[0]);
}
// k_pos_hash_w with the witness written out: the complete assignment of zl_circuit_poseidon_hash(curve, W - 1, in) per item, one lane each.  Row p = out +
// p * stride elements (16-byte aligned): [0] = 1, [1] = the digest, [2 .. W + 1) the inputs, then the 3 (8 W + partial - 1) records of the hash; elements
// behind them are not touched.  The inputs are copied before the permutation (rows and inputs do not overlap), [0] and [1] go out last.  pub (may be null)
// receives the digest, densely.  At W = 3 the row is k_pos_chain_trace's for k = 1: the same permutation (permute_any), the same recorder, the same layout.
template <class FrP, int W>
__global__ __launch_bounds__(BLOCK) void k_pos_hash_trace(const uint32_t* __restrict__ tab, const uint64_t* __restrict__ in, size_t n, uint64_t* __restrict__ out,
                                                          size_t stride, uint64_t* __restrict__ pub, uint32_t* __restrict__ flag) {
    const size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint64_t* x = in + p * (4 * (W - 1));
    uint64_t* row = out + p * stride * 4;
    El<FrP> s[W];
    s[0] = tab_ld<FrP>(tab, pd::tab_tag(W));
    bool ok = true;
#pragma unroll
    for (int i = 1; i < W; i++) {
        const uint64_t* xi = x + 4 * (i - 1);
        ok &= dload<FrP>(xi, s[i]);
        copy16(row + 4 * (i + 1), xi[0], xi[1], xi[2], xi[3]);
    }
    if (!ok) atomicOr(flag, 1u);
    RowRec<FrP> rec{row + 4 * (W + 1)};
    permute_any<FrP, W>(tab, s, rec);
    copy16(row, 1, 0, 0, 0);
    dstore16<FrP>(row + 4, s[0]);
    if (pub) dstore<FrP>(pub + p * 4, s[0]);
}
// The hand-over from the wide permutation into the width-3 levels of k_pos_leaf_merkle_trace.  The leaf digest is element 0 of the wide permutation's output:
// a row sum below ROW r = 2 W r (8, 10, 12).  The width-3 unit's argument (above LazyP) takes a state element entering a round at < 6r; an unreduced
// digest plus its round key would be squared at (ROW + 2)^2 = 100, 144, 196 -- above MUL_BOUND on BLS12-381 at every width and on BN254 at width 6.  So the
// digest is reduced weakly (wred: below 128 r in, < 2r out) before it becomes `cur`, at every width above 3 and on both fields: the bound holds by
// construction, not because inputs happen to stay small.  At width 3 the digest is the row sum of three products (< 6r), the running digest k_pos_merkle_trace
// has, and goes over as it is.
template <class FrP, int W>
struct HandOver {
    static constexpr int LEVEL_IN = 6;                         // what the width-3 unit's argument assumes of a state element entering a round
    static constexpr int DIGEST = WideBounds<FrP, W>::ROW;     // the wide permutation's output
    static constexpr bool REDUCE = DIGEST > LEVEL_IN;
    static constexpr int CUR = REDUCE ? 2 : DIGEST;            // what enters the first level as left or right
    static constexpr int LEVEL_SQ = (CUR + 2) * (CUR + 2);     // x^2 of it plus a round key
    static_assert(DIGEST <= 128, "wred takes a value below 128 r");
    static_assert(CUR <= LEVEL_IN && LEVEL_SQ <= 64 && LEVEL_SQ <= LazyP<FrP>::P::MUL_BOUND, "the width-3 levels take their first running digest within their bound");
};
#define ZL_POS_HAND_OVER(FrP, W, reduce, cur) static_assert(HandOver<FrP, W>::REDUCE == reduce && HandOver<FrP, W>::CUR == cur, "hand-over of " #FrP " at width " #W)
ZL_POS_HAND_OVER(BLS12_381_Fr, 3, false, 6);  // a width-3 row sum: the running digest of k_pos_merkle_trace
ZL_POS_HAND_OVER(BLS12_381_Fr, 4, true, 2);   // 8 r: (8 + 2)^2 = 100 > 70
ZL_POS_HAND_OVER(BLS12_381_Fr, 5, true, 2);   // 10 r: 144 > 70
ZL_POS_HAND_OVER(BLS12_381_Fr, 6, true, 2);   // 12 r: 196 > 70
ZL_POS_HAND_OVER(BN254_Fr, 3, false, 6);
ZL_POS_HAND_OVER(BN254_Fr, 4, true, 2);       // 100 <= 169 would pass the square, but not the 6 r the levels' argument is written for
ZL_POS_HAND_OVER(BN254_Fr, 5, true, 2);
ZL_POS_HAND_OVER(BN254_Fr, 6, true, 2);       // 196 > 169
#undef ZL_POS_HAND_OVER
// Where k_pos_leaf_merkle_trace reads item p's preimage (`per` = W - 1 elements), the digest its hash must equal (nullptr: nothing to compare with) and its
// sibling at level k: explicit arrays, or a tree's node array beside the preimages of the tree's leaves, preimage of leaf i at element i * per.
struct LeafPathSrc {
    const uint64_t* preimages;
    const uint64_t* paths;
    unsigned depth;
    __device__ __forceinline__ const uint64_t* preimage(size_t p, uint64_t, unsigned per) const { return preimages + p * per * 4; }
    __device__ __forceinline__ const uint64_t* leaf_digest(uint64_t) const { return nullptr; }
    __device__ __forceinline__ const uint64_t* sibling(size_t p, uint64_t, unsigned k) const { return paths + (p * depth + k) * 4; }
    LeafPathSrc advanced(size_t first, unsigned per) const { return LeafPathSrc{preimages + first * per * 4, paths + first * depth * 4, depth}; }
};
struct LeafTreeSrc {
    const uint64_t* nodes;
    const uint64_t* preimages;
    LevelTable lt;
    __device__ __forceinline__ const uint64_t* preimage(size_t, uint64_t idx, unsigned per) const { return preimages + idx * per * 4; }
    __device__ __forceinline__ const uint64_t* leaf_digest(uint64_t idx) const { return nodes + idx * 4; }
    __device__ __forceinline__ const uint64_t* sibling(size_t, uint64_t idx, unsigned k) const {
        const uint64_t sib = (idx >> k) ^ 1;
        return sib < lt.size[k] ? nodes + (lt.off[k] + sib) * 4 : nullptr;
    }
    LeafTreeSrc advanced(size_t, unsigned) const { return *this; }
};
// The complete assignment of zl_circuit_poseidon_merkle_leaf(curve, W - 1, depth, preimage, index, path) per item, one lane each: the leaf hash through
// permute_any (tab: the table of width W), then `depth` levels through permute_dev (tab3: the width-3 table), exactly k_pos_merkle_trace's.  Row p = out +
// p * stride elements (16-byte aligned): [0] = 1, [1] = root, [2 .. W + 1) the preimage, the leaf hash's records, then level j at W + 1 + records + 238 j:
// [+0] sibling, [+1] index bit, [+2] left, [+3] right, [+4 .. +238) the records of H(left, right); nothing behind the row is touched.  The leaf digest is not
// part of the row (the circuit keeps it a linear combination); where the source knows the digest the tree holds for the leaf, a hash that differs from it sets
// bit 1 of the flag word -- the row would otherwise be a valid one for another root.  pub (may be null) receives the root, densely.
template <class FrP, int W, class Src>
__global__ __launch_bounds__(BLOCK) void k_pos_leaf_merkle_trace(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ tab3, const Src src,
                                                                 const uint64_t* __restrict__ indices, unsigned depth, size_t n, uint64_t* __restrict__ out, size_t stride,
                                                                 uint64_t* __restrict__ pub, uint32_t* __restrict__ flag) {
    const size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint64_t idx = indices[p];
    uint64_t* row = out + p * stride * 4;
    bool ok = true;
    El<FrP> cur;
    {
        const uint64_t* x = src.preimage(p, idx, W - 1);
        El<FrP> s[W];
        s[0] = tab_ld<FrP>(tab, pd::tab_tag(W));
#pragma unroll
        for (int i = 1; i < W; i++) {
            const uint64_t* xi = x + 4 * (i - 1);
            ok &= dload<FrP>(xi, s[i]);
            copy16(row + 4 * (i + 1), xi[0], xi[1], xi[2], xi[3]);
        }
        RowRec<FrP> rec{row + 4 * (W + 1)};
        permute_any<FrP, W>(tab, s, rec);
        if (const uint64_t* lw = src.leaf_digest(idx)) {
            uint64_t d[4];
            dstore<FrP>(d, s[0]);
            if (d[0] != lw[0] || d[1] != lw[1] || d[2] != lw[2] || d[3] != lw[3]) atomicOr(flag, 2u);
        }
        if constexpr (HandOver<FrP, W>::REDUCE) cur = zl::wred(s[0]);
        else cur = s[0];
    }
    uint64_t* lv = row + 4 * pd::hash_row_elems(W - 1);
#pragma unroll 1
    for (unsigned k = 0; k < depth; k++) {
        const uint64_t* sw = src.sibling(p, idx, k);
        El<FrP> sib = ezero<FrP>();
        if (sw) {
            ok &= dload<FrP>(sw, sib);
            copy16(lv, sw[0], sw[1], sw[2], sw[3]);
        } else {
            copy16(lv, 0, 0, 0, 0);
        }
        const bool right = (idx >> k) & 1;
        copy16(lv + 4, right ? 1 : 0, 0, 0, 0);
        El<FrP> s0 = tab_ld<FrP>(tab3, pd::tab_tag(3)), x, y;
#pragma unroll
        for (int w = 0; w < El<FrP>::L; w++) {
            x.l[w] = right ? sib.l[w] : cur.l[w];
            y.l[w] = right ? cur.l[w] : sib.l[w];
        }
        dstore16<FrP>(lv + 8, x);
        dstore16<FrP>(lv + 12, y);
        RowRec<FrP> rec{lv + 16};
        permute_dev<FrP>(tab3, s0, x, y, rec);
        cur = s0;
        lv += (size_t)pd::MERKLE_PER_LEVEL * 4;
    }
    if (!ok) atomicOr(flag, 1u);
    copy16(row, 1, 0, 0, 0);
    dstore16<FrP>(row + 4, cur);
    if (pub) dstore<FrP>(pub + p * 4, cur);
}

// ---------------------------------------------------------------------------------------------------------------- the duplex cipher (zl_poseidon_duplex_*)
// One lane per message, the whole dependent chain of SB + N permutations in one launch (include/zl_backend_ext.h states the construction).  Between two
// permutations the lane adds a block into the rate -- lanes 1 .. W - 1 -- or, decrypting, overwrites the rate with the ciphertext.  None of this is covered by
// the permutations' bound arguments (above LazyP and above WideBounds), which know a state element entering a round as a row sum (< ROW r = 2 W r) or a loaded
// element (< 2r) and never as their SUM.  In units of r:
//   * an absorbed lane is a row sum -- or, in front of the first permutation, a loaded element of the initial state -- plus a loaded element: < (ROW + 2) r = SUM r
//     (8, 10, 12, 14).  With a round key that would be (2 W + 4) r, squared 100 at width 3 against the 64 the width-3 unit is argued for and BLS12-381's
//     MUL_BOUND of 70.  So the sum is reduced weakly AT ONCE, on both fields and at every width: wred takes a carried value below 128 r (add carries) and returns
//     < 2r, and the lane enters the permutation as a loaded element does -- the bound holds by construction.  rate wred per permutation against 804 .. 2 616
//     products.  A lane that absorbs nothing (lane 0; the rate lanes of a padding zero, which is skipped, not added) stays the row sum it was;
//   * the stored ciphertext is that reduced sum: dstore's mul(x, 1) takes it at 2 * 1 and hands canon a product (< 2r);
//   * decrypting, the plaintext is c - state with c loaded (< 2r) and state a row sum (message blocks follow SB >= 2 permutations), carried: subk with the
//     biased limbs of 2^J r, 2^J >= ROW + 2 (J = 3 at width 3, 4 above), gives a value < (2 + 2^J) r = DIFF r (10, 18), which dstore takes at DIFF * 1;
//   * the lane overwritten with a loaded ciphertext element is < 2r: a loaded element again;
//   * the tag is lane 1 of the last permutation's output, a row sum: dstore takes it at ROW * 1, as k_pos_permute_w stores its outputs.
// Every output goes through dstore's canon; the tag comparison is on canonical words.
constexpr int ceil_log2(int v) { return v <= 1 ? 0 : 1 + ceil_log2((v + 1) / 2); }
template <class FrP, int W>
struct DuplexBounds {
    using P = typename LazyP<FrP>::P;
    static constexpr int ROW = WideBounds<FrP, W>::ROW;      // a lane after a permutation
    static constexpr int LOADED = 2;                         // dload's product
    static constexpr int SUM = ROW + LOADED;                 // what wred sees (the first block: LOADED + LOADED)
    static constexpr int ABSORBED = 2;                       // ... and returns: the lane that enters the permutation
    static constexpr int CIPHER_STORE_MUL = ABSORBED * 1;
    static constexpr int SUB_J = ceil_log2(ROW + 2);         // the bias 2^J r of c - state
    static constexpr int DIFF = LOADED + (1 << SUB_J);
    static constexpr int PLAIN_STORE_MUL = DIFF * 1;
    static constexpr int OVERWRITTEN = LOADED;
    static constexpr int TAG_STORE_MUL = ROW * 1;
    static constexpr int MAX_MUL = cmax(CIPHER_STORE_MUL, cmax(PLAIN_STORE_MUL, TAG_STORE_MUL));
    static_assert(SUM <= 128 && DIFF <= 128, "wred and canon take a value below 128 r");
    static_assert((1 << SUB_J) >= ROW + 2 && SUB_J <= P::KQ_MAX, "subk: the bias covers the subtrahend, and the table holds it");
    static_assert(ABSORBED <= LOADED && OVERWRITTEN <= LOADED, "a rate lane enters the permutation within the bound of a loaded element");
    static_assert(MAX_MUL <= P::MUL_BOUND, "a bound product above what mul takes");
};
#define ZL_POS_DUPLEX_BOUNDS(FrP, W, sum, j, diff) \
    static_assert(DuplexBounds<FrP, W>::SUM == sum && DuplexBounds<FrP, W>::SUB_J == j && DuplexBounds<FrP, W>::DIFF == diff && DuplexBounds<FrP, W>::MAX_MUL == diff && \
                  DuplexBounds<FrP, W>::MAX_MUL <= LazyP<FrP>::P::MUL_BOUND, "duplex bounds of " #FrP " at width " #W)
ZL_POS_DUPLEX_BOUNDS(BLS12_381_Fr, 3, 8, 3, 10);   // unreduced: (8 + 2)^2 = 100 > 70
ZL_POS_DUPLEX_BOUNDS(BLS12_381_Fr, 4, 10, 4, 18);
ZL_POS_DUPLEX_BOUNDS(BLS12_381_Fr, 5, 12, 4, 18);
ZL_POS_DUPLEX_BOUNDS(BLS12_381_Fr, 6, 14, 4, 18);
ZL_POS_DUPLEX_BOUNDS(BN254_Fr, 3, 8, 3, 10);       // 100 <= 169 would pass the square, but not the 6 r the width-3 argument is written for
ZL_POS_DUPLEX_BOUNDS(BN254_Fr, 4, 10, 4, 18);
ZL_POS_DUPLEX_BOUNDS(BN254_Fr, 5, 12, 4, 18);
ZL_POS_DUPLEX_BOUNDS(BN254_Fr, 6, 14, 4, 18);
#undef ZL_POS_DUPLEX_BOUNDS
// the initial state, canonical words, by value in the kernel's arguments: wave-uniform loads, nothing to stage
struct DuplexInit {
    uint64_t w[4 * pd::MAX_WIDTH];
};
// rate lanes I .. W - 2 of one block, one after the other (a compile-time recursion for the reason sbox_lanes gives: the state keeps static indices).  Lane i
// takes element i of the block when i < avail: a setup block is added; a message block is added and stored (encrypt) or subtracted from, stored and
// overwritten (decrypt).  src and dst may be the same address: element i is read before it is written.
template <class FrP, int W, int I>
__device__ __forceinline__ void duplex_lanes(El<FrP> (&s)[W], const uint64_t* src, uint64_t* dst, uint32_t avail, bool message, bool decrypt, bool& ok) {
    if constexpr (I < W - 1) {
        using P = typename LazyP<FrP>::P;
        if ((uint32_t)I < avail) {
            El<FrP> e;
            ok &= dload<FrP>(src + 4 * I, e);
            El<FrP> nx = zl::wred(zl::add(s[1 + I], e));
            if (message) {
                El<FrP> o = nx;
                if (decrypt) {
                    uint32_t K[P::L];
#pragma unroll
                    for (int k = 0; k < P::L; k++) K[k] = P::kq(DuplexBounds<FrP, W>::SUB_J, k);
                    o = zl::subk(e, s[1 + I], K);
                    nx = e;
                }
                dstore<FrP>(dst + 4 * I, o);
            }
            s[1 + I] = nx;
        }
        duplex_lanes<FrP, W, I + 1>(s, src, dst, avail, message, decrypt, ok);
    }
}
// Message p: K key elements at keys + p K, H header elements, N blocks of W - 1 text elements at text_in + p N (W - 1), written to the same offset of text_out
// (which may BE text_in).  Block t of the lane's SB + N is a key block (t < kb = K / rate + 1), a header block (t < sb) or a message block; all of it is
// wave-uniform, as is `decrypt`.  Encrypting, tags[p] receives the tag; decrypting, tags[p] is read and ok_each[p] = 1 when it equals the computed one.
template <class FrP, int W>
__global__ __launch_bounds__(BLOCK) void k_pos_duplex(const uint32_t* __restrict__ tab, const DuplexInit init, const uint64_t* __restrict__ keys, uint32_t K,
                                                      const uint64_t* __restrict__ headers, uint32_t H, const uint64_t* text_in, uint32_t N, size_t n, uint64_t* text_out,
                                                      uint64_t* tags, uint8_t* __restrict__ ok_each, bool decrypt, uint32_t* __restrict__ flag) {
    const size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    constexpr uint32_t RATE = W - 1;
    El<FrP> s[W];
#pragma unroll
    for (int i = 0; i < W; i++) (void)dload<FrP>(init.w + 4 * i, s[i]);  // (checked on the host)
    const uint32_t kb = K / RATE + 1, sb = kb + H / RATE + 1, total = sb + N;
    const uint64_t* key = keys + p * K * 4;
    const uint64_t* header = headers + p * H * 4;
    const uint64_t* tin = text_in + p * N * RATE * 4;
    uint64_t* tout = text_out + p * N * RATE * 4;
    bool ok = true;
    NoRec none;
#pragma unroll 1
    for (uint32_t t = 0; t < total; t++) {
        const bool message = t >= sb;
        const uint32_t b = message ? t - sb : t < kb ? t : t - kb;       // the block's number within its sequence
        const uint32_t len = message ? N * RATE : t < kb ? K : H;         // ... and the sequence's length: b * RATE <= len
        const uint64_t* src = (message ? tin : t < kb ? key : header) + (size_t)b * RATE * 4;
        const uint32_t left = len - b * RATE;
        duplex_lanes<FrP, W, 0>(s, src, tout + (size_t)b * RATE * 4, left < RATE ? left : RATE, message, decrypt, ok);
        permute_any<FrP, W>(tab, s, none);
    }
    uint64_t tg[4];
    dstore<FrP>(tg, s[1]);
    uint64_t* tag = tags + p * 4;
    if (decrypt) {
        ok &= canon_words<FrP>(tag);
        ok_each[p] = tg[0] == tag[0] && tg[1] == tag[1] && tg[2] == tag[2] && tg[3] == tag[3];
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) tag[i] = tg[i];
    }
    if (!ok) atomicOr(flag, 1u);
}
// ---- the encryption with its witness written out (zl_poseidon_encrypt_assignments): k_pos_duplex's chain, encrypting, under a recorder.
// What the trace stores that k_pos_duplex does not, in units of r:
//   * the records x^2, x^4, x^5 of an S-box: products (< 2r) whichever way the input came (with WideBounds::REDUCE: of the reduced input, the same element);
//     the canonical store's mul(x, 1) takes them at 2 * 1, as in every trace kernel;
//   * the public ciphertext cell: the absorbed lane, wred's result (< ABSORBED r = 2r) -- the value k_pos_duplex stores as the ciphertext, at 2 * 1;
//   * the tag cell: lane 1 of the last permutation's output, a row sum, at ROW * 1 as k_pos_duplex's tag;
//   * key, header and plaintext cells are the input words copied as they are (an input >= r raises the flag and the call fails).
// Recording reads the S-box's intermediates and changes none of them: every bound of DuplexBounds and of the permutations holds unchanged.  The permutations
// after the first enter round 0 with lane 0 a row sum (< ROW r) plus a round key -- what WideBounds (KEYED) and the width-3 argument (< 6r entering a round)
// already assume of any lane; that its S-box is now RECORDED there changes no operand.
template <class FrP, int W>
struct DuplexTraceBounds {
    using P = typename LazyP<FrP>::P;
    static constexpr int RECORD = 2;                                             // a product
    static constexpr int RECORD_STORE_MUL = RECORD * 1;
    static constexpr int CIPHER_CELL_MUL = DuplexBounds<FrP, W>::ABSORBED * 1;   // the reduced sum
    static constexpr int TAG_CELL_MUL = DuplexBounds<FrP, W>::TAG_STORE_MUL;
    static constexpr int MAX_MUL = cmax(RECORD_STORE_MUL, cmax(CIPHER_CELL_MUL, TAG_CELL_MUL));
    static_assert(MAX_MUL <= P::MUL_BOUND, "a bound product above what mul takes");
    static_assert(RECORD <= 128 && DuplexBounds<FrP, W>::ABSORBED <= 128 && WideBounds<FrP, W>::ROW <= 128, "canon takes a value below 128 r");
};
#define ZL_POS_DUPLEX_TRACE_BOUNDS(FrP, W, tag_mul) \
    static_assert(DuplexTraceBounds<FrP, W>::RECORD_STORE_MUL == 2 && DuplexTraceBounds<FrP, W>::CIPHER_CELL_MUL == 2 && DuplexTraceBounds<FrP, W>::TAG_CELL_MUL == tag_mul && \
                  DuplexTraceBounds<FrP, W>::MAX_MUL == tag_mul && DuplexTraceBounds<FrP, W>::MAX_MUL <= LazyP<FrP>::P::MUL_BOUND, "duplex trace bounds of " #FrP " at width " #W)
ZL_POS_DUPLEX_TRACE_BOUNDS(BLS12_381_Fr, 3, 6);
ZL_POS_DUPLEX_TRACE_BOUNDS(BLS12_381_Fr, 4, 8);
ZL_POS_DUPLEX_TRACE_BOUNDS(BLS12_381_Fr, 5, 10);
ZL_POS_DUPLEX_TRACE_BOUNDS(BLS12_381_Fr, 6, 12);
ZL_POS_DUPLEX_TRACE_BOUNDS(BN254_Fr, 3, 6);
ZL_POS_DUPLEX_TRACE_BOUNDS(BN254_Fr, 4, 8);
ZL_POS_DUPLEX_TRACE_BOUNDS(BN254_Fr, 5, 10);
ZL_POS_DUPLEX_TRACE_BOUNDS(BN254_Fr, 6, 12);
#undef ZL_POS_DUPLEX_TRACE_BOUNDS
// The round-0 lanes the encryption circuit does NOT record in its first permutation: lane 0 (the capacity constant) and the rate lanes without a key element,
// 1 + K .. W - 1 when K < rate -- their input is a constant of the initial state plus a round key whatever that constant is.  Later permutations: none.
ZL_HD uint32_t rec0_mask(unsigned width, size_t key_len, bool first) {
    if (!first) return 0u;
    const unsigned kk = key_len < width - 1 ? (unsigned)key_len : width - 1;
    return 1u | (((1u << width) - 1u) ^ ((1u << (1 + kk)) - 1u));
}
// rate lanes I .. W - 2 of one block under the trace (duplex_lanes, encrypting): lane i takes element i of the block when i < avail, the element's words go to
// cell i of `in_cells` (16-byte aligned) as they are -- unless `copy` is false: the block is read from the row's own cells (a key another circuit's launch
// left there) -- and a message block's reduced sum -- the ciphertext -- to cell i of ct_cells and, densely, to ct_pub (may be null): one canonical store,
// written twice.
template <class FrP, int W, int I>
__device__ __forceinline__ void duplex_trace_lanes(El<FrP> (&s)[W], const uint64_t* src, uint64_t* in_cells, uint64_t* ct_cells, uint64_t* ct_pub, uint32_t avail, bool message,
                                                   bool copy, bool& ok) {
    if constexpr (I < W - 1) {
        if ((uint32_t)I < avail) {
            const uint64_t* x = src + 4 * I;
            El<FrP> e;
            ok &= dload<FrP>(x, e);
            if (copy) copy16(in_cells + 4 * I, x[0], x[1], x[2], x[3]);
            s[1 + I] = zl::wred(zl::add(s[1 + I], e));
            if (message) {
                uint64_t c[4];
                dstore<FrP>(c, s[1 + I]);
                copy16(ct_cells + 4 * I, c[0], c[1], c[2], c[3]);
                if (ct_pub) {
#pragma unroll
                    for (int k = 0; k < 4; k++) ct_pub[4 * I + k] = c[k];
                }
            }
        }
        duplex_trace_lanes<FrP, W, I + 1>(s, src, in_cells, ct_cells, ct_pub, avail, message, copy, ok);
    }
}
// Where one lane's row keeps the cipher's cells (16-byte aligned each), and where its key is read from.  The row-layout descriptor of the trace body: the
// encryption circuit's own row (k_pos_duplex_trace) and a row of a circuit that holds the cipher inside it (k_pos_duplex_trace_in: zl_duplex_row_layout).
struct DuplexRowCells {
    uint64_t *one, *tag, *ct, *header, *key, *plain, *rec;  // one: [0] = 1 is written there, or null; key: where the key is copied TO (unused when KEY_IN_ROW)
    const uint64_t* key_from;                               // K elements: the call's keys, or cells of the row itself
};
// The body of both trace kernels, one lane a row: k_pos_duplex's chain, encrypting, under a recorder.  The lane writes the input cells and the ciphertext
// cells as it absorbs their blocks, the records as the permutations run, [0] and the tag last.  KEY_IN_ROW: the key blocks are read from the row and copied
// nowhere.  tag_pub / ct_pub (may be null): the lane's dense tag and ciphertext.  K >= 1; block selection as in k_pos_duplex, all wave-uniform, and so is the
// record mask.  No new arithmetic over DuplexTraceBounds: a key read from the row is a canonical element like one read from the call's keys.
template <class FrP, int W, bool KEY_IN_ROW>
__device__ __forceinline__ void duplex_trace_row(const uint32_t* __restrict__ tab, const DuplexInit& init, const DuplexRowCells& c, uint32_t K, const uint64_t* header, uint32_t H,
                                                 const uint64_t* text, uint32_t N, uint64_t* tag_pub, uint64_t* ct_pub, uint32_t* __restrict__ flag) {
    constexpr uint32_t RATE = W - 1;
    El<FrP> s[W];
#pragma unroll
    for (int i = 0; i < W; i++) (void)dload<FrP>(init.w + 4 * i, s[i]);  // (checked on the host)
    const uint32_t kb = K / RATE + 1, sb = kb + H / RATE + 1, total = sb + N, T = N * RATE;
    RowRec<FrP> rec{c.rec};
    bool ok = true;
#pragma unroll 1
    for (uint32_t t = 0; t < total; t++) {
        const bool message = t >= sb;
        const uint32_t b = message ? t - sb : t < kb ? t : t - kb;       // the block's number within its sequence
        const uint32_t len = message ? T : t < kb ? K : H;                // ... and the sequence's length: b * RATE <= len
        const size_t at = (size_t)b * RATE * 4;
        const uint64_t* src = (message ? text : t < kb ? c.key_from : header) + at;
        uint64_t* in_cells = (message ? c.plain : t < kb ? c.key : c.header) + at;
        const uint32_t left = len - b * RATE;
        duplex_trace_lanes<FrP, W, 0>(s, src, in_cells, message ? c.ct + at : nullptr, message && ct_pub ? ct_pub + at : nullptr, left < RATE ? left : RATE, message,
                                      !KEY_IN_ROW || t >= kb, ok);
        permute_any<FrP, W>(tab, s, rec, rec0_mask(W, K, t == 0));
    }
    if (!ok) atomicOr(flag, 1u);
    uint64_t tg[4];
    dstore<FrP>(tg, s[1]);
    if (!KEY_IN_ROW) copy16(c.one, 1, 0, 0, 0);
    copy16(c.tag, tg[0], tg[1], tg[2], tg[3]);
    if (tag_pub) {
#pragma unroll
        for (int i = 0; i < 4; i++) tag_pub[i] = tg[i];
    }
}
// k_pos_duplex, encrypting, with the witness written out: the complete assignment of zl_circuit_poseidon_encrypt(curve, W, init, key, header, plaintext) per
// message, one lane each, the SB + N dependent permutations in one launch.  Row p = out + p * stride elements (16-byte aligned), rate = W - 1:
//   [0] = 1   [1] = tag   [2 .. 2 + N rate) ciphertext   [.. + H) header   [.. + K) key   [.. + N rate) plaintext   then 3 S record elements in execution order;
// elements behind the row are not touched.  Rows and inputs do not overlap.  tags / cts (may be null) receive the tag and the N rate ciphertext elements,
// densely.  The body is duplex_trace_row's.
template <class FrP, int W>
__global__ __launch_bounds__(BLOCK) void k_pos_duplex_trace(const uint32_t* __restrict__ tab, const DuplexInit init, const uint64_t* __restrict__ keys, uint32_t K,
                                                            const uint64_t* __restrict__ headers, uint32_t H, const uint64_t* __restrict__ texts, uint32_t N, size_t n,
                                                            uint64_t* __restrict__ out, size_t stride, uint64_t* __restrict__ tags, uint64_t* __restrict__ cts,
                                                            uint32_t* __restrict__ flag) {
    const size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint32_t T = N * (W - 1);
    uint64_t* row = out + p * stride * 4;
    DuplexRowCells c;
    c.one = row;
    c.tag = row + 4;
    c.ct = row + 8;
    c.header = c.ct + (size_t)T * 4;
    c.key = c.header + (size_t)H * 4;
    c.plain = c.key + (size_t)K * 4;
    c.rec = c.plain + (size_t)T * 4;
    c.key_from = keys + p * K * 4;
    duplex_trace_row<FrP, W, false>(tab, init, c, K, headers + p * H * 4, H, texts + p * T * 4, N, tags ? tags + p * 4 : nullptr, cts ? cts + p * T * 4 : nullptr, flag);
}
// The same body inside another circuit's rows (zl_poseidon_duplex_row_launch; zl_circuit_hybrid_encrypt's: the key is the agreed point the pk ladder of
// k_ed_hybrid_ladders left in the row, earlier on the stream).  lay: element offsets within the row; [0] is not written; the key is read from the row, so
// `out` is read and written and carries no __restrict__.
template <class FrP, int W>
__global__ __launch_bounds__(BLOCK) void k_pos_duplex_trace_in(const uint32_t* __restrict__ tab, const DuplexInit init, const zl_duplex_row_layout lay, uint32_t K,
                                                               const uint64_t* __restrict__ headers, uint32_t H, const uint64_t* __restrict__ texts, uint32_t N, size_t n,
                                                               uint64_t* out, size_t stride, uint64_t* __restrict__ tags, uint64_t* __restrict__ cts,
                                                               uint32_t* __restrict__ flag) {
    const size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint32_t T = N * (W - 1);
    uint64_t* row = out + p * stride * 4;
    DuplexRowCells c;
    c.one = nullptr;
    c.tag = row + lay.tag * 4;
    c.ct = row + lay.ct * 4;
    c.header = row + lay.header * 4;
    c.key = nullptr;
    c.plain = row + lay.plain * 4;
    c.rec = row + lay.rec * 4;
    c.key_from = row + lay.key * 4;
    duplex_trace_row<FrP, W, true>(tab, init, c, K, headers + p * H * 4, H, texts + p * T * 4, N, tags ? tags + p * 4 : nullptr, cts ? cts + p * T * 4 : nullptr, flag);
}

// ---------------------------------------------------------------------------------------------------------------- host path
template <class FrP, int W = 3>
const poseidon::Constants<FrP, W>& consts() {
    static const poseidon::Constants<FrP, W> c;
    return c;
}
template <class FrP>
bool host_hash2(const uint64_t* x, const uint64_t* y, uint64_t* out) {  // y == nullptr: the zero digest
    Fp<FrP> st[3] = {zl::from_u64<FrP>(3), Fp<FrP>::zero(), Fp<FrP>::zero()};
    bool ok = load_canon<FrP>(x, st[1]);
    if (y) ok &= load_canon<FrP>(y, st[2]);
    poseidon::permute_native(consts<FrP>(), st);
    store_canon<FrP>(out, st[0]);
    return ok;
}
// f(0) .. f(n - 1) over the host pool in blocks; false when any f returned false
template <class Fn>
bool host_for(size_t n, const Fn& f) {
    constexpr size_t B = 32;
    std::atomic<int> bad{0};
    const std::function<void(size_t)> g = [&](size_t b) {
        const size_t end = (b + 1) * B < n ? (b + 1) * B : n;
        bool ok = true;
        for (size_t i = b * B; i < end; i++) ok &= f(i);
        if (!ok) bad.store(1);
    };
    zl_pool_get().parallel_for((n + B - 1) / B, g);
    return bad.load() == 0;
}
// the batched permutation and hash at width W: the host mirror's permute_native on the constants of the width
template <class FrP, int W>
int host_permute_w(uint64_t* states, size_t count) {
    consts<FrP, W>();  // (built before the pool's threads ask for it)
    return host_for(count, [&](size_t i) {
        Fp<FrP> st[W];
        bool ok = true;
        for (int e = 0; e < W; e++) ok &= load_canon<FrP>(states + i * (4 * W) + 4 * e, st[e]);
        poseidon::permute_native(consts<FrP, W>(), st);
        for (int e = 0; e < W; e++) store_canon<FrP>(states + i * (4 * W) + 4 * e, st[e]);
        return ok;
    }) ? ZL_OK : ZL_EINVAL;
}
template <class FrP, int W>
int host_hash_w(const uint64_t* in, size_t count, uint64_t* out) {
    consts<FrP, W>();
    return host_for(count, [&](size_t i) {
        Fp<FrP> st[W];
        st[0] = zl::from_u64<FrP>(pd::spec_of_width(W).tag);
        bool ok = true;
        for (int e = 1; e < W; e++) ok &= load_canon<FrP>(in + i * (4 * (W - 1)) + 4 * (e - 1), st[e]);
        poseidon::permute_native(consts<FrP, W>(), st);
        store_canon<FrP>(out + i * 4, st[0]);
        return ok;
    }) ? ZL_OK : ZL_EINVAL;
}
// one state on the calling thread (zl_poseidon_permute_w) and the constants themselves, canonical (zl_poseidon_constants)
template <class FrP, int W>
int host_permute_one(uint64_t* state) {
    Fp<FrP> st[W];
    for (int i = 0; i < W; i++) {  // (as zl_poseidon_permute: the words are taken as they are, a value >= r counts mod r)
        memcpy(st[i].l, state + 4 * i, 32);
        st[i] = zl::to_mont(st[i]);
    }
    poseidon::permute_native(consts<FrP, W>(), st);
    for (int i = 0; i < W; i++) store_canon<FrP>(state + 4 * i, st[i]);
    return ZL_OK;
}
template <class FrP, int W>
int constants_out(uint64_t* keys, uint64_t* mds) {
    const poseidon::Constants<FrP, W>& c = consts<FrP, W>();
    if (keys)
        for (size_t i = 0; i < c.round_keys.size(); i++) store_canon<FrP>(keys + 4 * i, c.round_keys[i]);
    if (mds)
        for (int i = 0; i < W; i++)
            for (int j = 0; j < W; j++) store_canon<FrP>(mds + 4 * (W * i + j), c.mds[i][j]);
    return ZL_OK;
}
template <class FrP>
int host_chain(const uint64_t* x0, const uint64_t* x1, uint32_t k, size_t count, uint64_t* out) {
    consts<FrP>();
    return host_for(count, [&](size_t i) {
        Fp<FrP> h, b;
        bool ok = load_canon<FrP>(x0 + i * 4, h);
        ok &= load_canon<FrP>(x1 + i * 4, b);
        for (uint32_t j = 0; j < k; j++) {
            Fp<FrP> st[3] = {zl::from_u64<FrP>(3), h, b};
            poseidon::permute_native(consts<FrP>(), st);
            h = st[0];
        }
        store_canon<FrP>(out + i * 4, h);
        return ok;
    }) ? ZL_OK : ZL_EINVAL;
}
// row i = the assignment of chain i (nv = 4 + 234 k elements): what poseidon_chain_witness allocates, through permute_native_record
template <class FrP>
int host_assignments(const uint64_t* x0, const uint64_t* x1, uint32_t k, size_t count, uint64_t* out, size_t nv) {
    consts<FrP>();
    return host_for(count, [&](size_t i) {
        Fp<FrP> h, b;
        bool ok = load_canon<FrP>(x0 + i * 4, h);
        ok &= load_canon<FrP>(x1 + i * 4, b);
        uint64_t* row = out + i * nv * 4;
        std::vector<Fp<FrP>> rec;  // one link at a time: 234 elements, whatever k is
        rec.reserve(pd::TRACE_PER_LINK);
        for (uint32_t j = 0; j < k; j++) {
            Fp<FrP> st[3] = {zl::from_u64<FrP>(3), h, b};
            rec.clear();
            poseidon::permute_native_record(consts<FrP>(), st, rec);
            h = st[0];
            uint64_t* link = row + 16 + (size_t)j * pd::TRACE_PER_LINK * 4;
            for (size_t t = 0; t < rec.size(); t++) store_canon<FrP>(link + 4 * t, rec[t]);
        }
        row[0] = 1;
        row[1] = row[2] = row[3] = 0;
        store_canon<FrP>(row + 4, h);
        memcpy(row + 8, x0 + i * 4, 32);
        memcpy(row + 12, x1 + i * 4, 32);
        return ok;
    }) ? ZL_OK : ZL_EINVAL;
}
// every level into `nodes` (level 0 = the leaves)
template <class FrP>
int host_merkle(const uint64_t* leaves, size_t n, unsigned depth, uint64_t* nodes) {
    consts<FrP>();
    if (n && nodes != leaves) memcpy(nodes, leaves, n * 32);
    bool ok = true;
    size_t off = 0, cm = n;
    for (unsigned k = 1; k <= depth && cm; k++) {
        const size_t pm = (cm + 1) / 2;
        const uint64_t* child = nodes + off * 4;
        uint64_t* parent = nodes + (off + cm) * 4;
        ok &= host_for(pm, [&](size_t j) { return host_hash2<FrP>(child + 2 * j * 4, 2 * j + 1 < cm ? child + (2 * j + 1) * 4 : nullptr, parent + j * 4); });
        off += cm;
        cm = pm;
    }
    return ok ? ZL_OK : ZL_EINVAL;
}
template <class FrP>
int host_fold(const uint64_t* leaves, const uint64_t* indices, const uint64_t* paths, unsigned depth, size_t count, uint64_t* roots) {
    consts<FrP>();
    return host_for(count, [&](size_t i) {
        uint64_t cur[4];
        memcpy(cur, leaves + i * 4, 32);
        bool ok = true;
        for (unsigned k = 0; k < depth; k++) {
            const uint64_t* sib = paths + (i * depth + k) * 4;
            uint64_t nx[4];
            ok &= ((indices[i] >> k) & 1) ? host_hash2<FrP>(sib, cur, nx) : host_hash2<FrP>(cur, sib, nx);
            memcpy(cur, nx, 32);
        }
        memcpy(roots + i * 4, cur, 32);
        return ok;
    }) ? ZL_OK : ZL_EINVAL;
}
// row i = the assignment of membership i (nv = 3 + 238 depth elements): what poseidon_merkle_witness allocates, level after level through permute_native_record
template <class FrP>
int host_merkle_assignments(const uint64_t* leaves, const uint64_t* indices, const uint64_t* paths, unsigned depth, size_t count, uint64_t* out, size_t nv) {
    consts<FrP>();
    return host_for(count, [&](size_t i) {
        Fp<FrP> cur;
        bool ok = load_canon<FrP>(leaves + i * 4, cur);
        uint64_t* row = out + i * nv * 4;
        memcpy(row + 8, leaves + i * 4, 32);
        std::vector<Fp<FrP>> rec;
        rec.reserve(pd::TRACE_PER_LINK);
        for (unsigned k = 0; k < depth; k++) {
            const uint64_t* sw = paths + (i * depth + k) * 4;
            uint64_t* lv = row + 12 + (size_t)k * pd::MERKLE_PER_LEVEL * 4;
            Fp<FrP> sib;
            ok &= load_canon<FrP>(sw, sib);
            const bool right = (indices[i] >> k) & 1;
            memcpy(lv, sw, 32);
            lv[4] = right ? 1 : 0;
            lv[5] = lv[6] = lv[7] = 0;
            Fp<FrP> st[3] = {zl::from_u64<FrP>(3), right ? sib : cur, right ? cur : sib};
            store_canon<FrP>(lv + 8, st[1]);
            store_canon<FrP>(lv + 12, st[2]);
            rec.clear();
            poseidon::permute_native_record(consts<FrP>(), st, rec);
            cur = st[0];
            for (size_t t = 0; t < rec.size(); t++) store_canon<FrP>(lv + 16 + 4 * t, rec[t]);
        }
        row[0] = 1;
        row[1] = row[2] = row[3] = 0;
        store_canon<FrP>(row + 4, cur);
        return ok;
    }) ? ZL_OK : ZL_EINVAL;
}
// the leaf hash of the two arity-general rows: inputs at row[2 ..), the records behind them; returns the digest (Montgomery) in *digest
template <class FrP, int W>
bool host_hash_records(const uint64_t* in, uint64_t* row, Fp<FrP>* digest) {
    Fp<FrP> st[W];
    st[0] = zl::from_u64<FrP>(pd::spec_of_width(W).tag);
    bool ok = true;
    for (int e = 1; e < W; e++) ok &= load_canon<FrP>(in + 4 * (e - 1), st[e]);
    memcpy(row + 8, in, 32 * (W - 1));
    std::vector<Fp<FrP>> rec;
    rec.reserve(pd::trace_per_hash(W - 1));
    poseidon::permute_native_record(consts<FrP, W>(), st, rec);
    for (size_t t = 0; t < rec.size(); t++) store_canon<FrP>(row + 4 * (W + 1) + 4 * t, rec[t]);
    *digest = st[0];
    return ok;
}
// row i = the assignment of hash circuit i (2 + arity + 3 S(arity) elements): what poseidon_arity allocates at depth 0
template <class FrP, int W>
int host_hash_assignments(const uint64_t* in, size_t count, uint64_t* out) {
    consts<FrP, W>();
    constexpr size_t nv = pd::hash_row_elems(W - 1);
    return host_for(count, [&](size_t i) {
        uint64_t* row = out + i * nv * 4;
        Fp<FrP> h;
        const bool ok = host_hash_records<FrP, W>(in + i * (4 * (W - 1)), row, &h);
        row[0] = 1;
        row[1] = row[2] = row[3] = 0;
        store_canon<FrP>(row + 4, h);
        return ok;
    }) ? ZL_OK : ZL_EINVAL;
}
// row i = the assignment of leaf membership i: the leaf hash as above, then the levels of host_merkle_assignments over its digest
template <class FrP, int W>
int host_leaf_assignments(const uint64_t* preimages, const uint64_t* indices, const uint64_t* paths, unsigned depth, size_t count, uint64_t* out) {
    consts<FrP, W>();
    consts<FrP>();
    const size_t nv = pd::leaf_row_elems(W - 1, depth);
    return host_for(count, [&](size_t i) {
        uint64_t* row = out + i * nv * 4;
        Fp<FrP> cur;
        bool ok = host_hash_records<FrP, W>(preimages + i * (4 * (W - 1)), row, &cur);
        std::vector<Fp<FrP>> rec;
        rec.reserve(pd::TRACE_PER_LINK);
        for (unsigned k = 0; k < depth; k++) {
            const uint64_t* sw = paths + (i * depth + k) * 4;
            uint64_t* lv = row + (pd::hash_row_elems(W - 1) + (size_t)k * pd::MERKLE_PER_LEVEL) * 4;
            Fp<FrP> sib;
            ok &= load_canon<FrP>(sw, sib);
            const bool right = (indices[i] >> k) & 1;
            memcpy(lv, sw, 32);
            lv[4] = right ? 1 : 0;
            lv[5] = lv[6] = lv[7] = 0;
            Fp<FrP> st[3] = {zl::from_u64<FrP>(3), right ? sib : cur, right ? cur : sib};
            store_canon<FrP>(lv + 8, st[1]);
            store_canon<FrP>(lv + 12, st[2]);
            rec.clear();
            poseidon::permute_native_record(consts<FrP>(), st, rec);
            cur = st[0];
            for (size_t t = 0; t < rec.size(); t++) store_canon<FrP>(lv + 16 + 4 * t, rec[t]);
        }
        row[0] = 1;
        row[1] = row[2] = row[3] = 0;
        store_canon<FrP>(row + 4, cur);
        return ok;
    }) ? ZL_OK : ZL_EINVAL;
}
// the duplex cipher over the host pool: the host mirror's duplex_encrypt / duplex_decrypt per message.  init: W canonical elements (checked by the caller).
// tags is written (encrypt) or read (decrypt, with ok_each written); text_out may be text_in -- a message is read whole before it is written.
template <class FrP, int W>
int host_duplex(const uint64_t* init, const uint64_t* keys, size_t K, const uint64_t* headers, size_t H, const uint64_t* text_in, size_t N, size_t count,
                uint64_t* text_out, uint64_t* tags, uint8_t* ok_each, bool decrypt) {
    consts<FrP, W>();
    const size_t T = N * (W - 1);
    Fp<FrP> st0[W];
    for (int e = 0; e < W; e++) (void)load_canon<FrP>(init + 4 * e, st0[e]);
    return host_for(count, [&](size_t i) {
        std::vector<Fp<FrP>> v(K + H + T);
        Fp<FrP>* key = v.data();
        Fp<FrP>* header = key + K;
        Fp<FrP>* text = header + H;
        bool ok = true;
        for (size_t e = 0; e < K; e++) ok &= load_canon<FrP>(keys + (i * K + e) * 4, key[e]);
        for (size_t e = 0; e < H; e++) ok &= load_canon<FrP>(headers + (i * H + e) * 4, header[e]);
        for (size_t e = 0; e < T; e++) ok &= load_canon<FrP>(text_in + (i * T + e) * 4, text[e]);
        Fp<FrP> st[W];
        for (int e = 0; e < W; e++) st[e] = st0[e];
        if (decrypt) {
            Fp<FrP> given;
            ok &= load_canon<FrP>(tags + i * 4, given);
            ok_each[i] = poseidon::duplex_decrypt<FrP, W>(consts<FrP, W>(), st, key, K, header, H, text, N) == given;
        } else {
            store_canon<FrP>(tags + i * 4, poseidon::duplex_encrypt<FrP, W>(consts<FrP, W>(), st, key, K, header, H, text, N));
        }
        for (size_t e = 0; e < T; e++) store_canon<FrP>(text_out + (i * T + e) * 4, text[e]);
        return ok;
    }) ? ZL_OK : ZL_EINVAL;
}
// One row of the encryption trace on the host, the mirror of duplex_trace_row: what poseidon_encrypt (zl_host.hip) allocates -- duplex_setup's and
// duplex_encrypt's block walk with permute_native_record in place of permute_native, under the circuit's round-0 mask (rec0_mask).  The header and plaintext
// cells hold their inputs already; the key is read from key_from (the row's key cells, or cells another circuit's gadget filled); the ciphertext cells, the
// records and the tag cell are written.  False for an element >= r.
template <class FrP, int W>
bool host_encrypt_row(const Fp<FrP> (&st0)[W], const uint64_t* key_from, size_t K, const uint64_t* h_cells, size_t H, const uint64_t* p_cells, size_t N, uint64_t* ct_cells,
                      uint64_t* rec_cells, uint64_t* tag_cell) {
    constexpr size_t rate = W - 1;
    Fp<FrP> st[W];
    for (int e = 0; e < W; e++) st[e] = st0[e];
    std::vector<Fp<FrP>> rec;
    rec.reserve(3 * (size_t)(consts<FrP, W>().FULL_ROUNDS * W + consts<FrP, W>().PARTIAL_ROUNDS));
    bool ok = true, first = true;
    auto permute = [&]() {
        rec.clear();
        poseidon::permute_native_record(consts<FrP, W>(), st, rec, rec0_mask(W, K, first));
        first = false;
        for (size_t t = 0; t < rec.size(); t++) store_canon<FrP>(rec_cells + 4 * t, rec[t]);
        rec_cells += 4 * rec.size();
    };
    for (int part = 0; part < 2; part++) {
        const uint64_t* src = part ? h_cells : key_from;
        const size_t len = part ? H : K;
        for (size_t b = 0; b <= len / rate; b++) {
            for (size_t l = 0; l < rate && b * rate + l < len; l++) {
                Fp<FrP> e;
                ok &= load_canon<FrP>(src + (b * rate + l) * 4, e);
                st[1 + l] = zl::add(st[1 + l], e);
            }
            permute();
        }
    }
    for (size_t j = 0; j < N; j++) {
        for (size_t l = 0; l < rate; l++) {
            Fp<FrP> e;
            ok &= load_canon<FrP>(p_cells + (j * rate + l) * 4, e);
            st[1 + l] = zl::add(st[1 + l], e);
            store_canon<FrP>(ct_cells + (j * rate + l) * 4, st[1 + l]);
        }
        permute();
    }
    store_canon<FrP>(tag_cell, st[1]);
    return ok;
}
// row i = the assignment of encryption i (nv = pd::encrypt_row_elems elements)
template <class FrP, int W>
int host_encrypt_assignments(const uint64_t* init, const uint64_t* keys, size_t K, const uint64_t* headers, size_t H, const uint64_t* texts, size_t N, size_t count,
                             uint64_t* out, size_t nv) {
    consts<FrP, W>();
    const size_t T = N * (W - 1);
    Fp<FrP> st0[W];
    for (int e = 0; e < W; e++) (void)load_canon<FrP>(init + 4 * e, st0[e]);
    return host_for(count, [&](size_t i) {
        uint64_t* row = out + i * nv * 4;
        uint64_t* ct_cells = row + 8;
        uint64_t* h_cells = ct_cells + T * 4;
        uint64_t* k_cells = h_cells + H * 4;
        uint64_t* p_cells = k_cells + K * 4;
        if (H) memcpy(h_cells, headers + i * H * 4, H * 32);
        memcpy(k_cells, keys + i * K * 4, K * 32);
        memcpy(p_cells, texts + i * T * 4, T * 32);
        row[0] = 1;
        row[1] = row[2] = row[3] = 0;
        return host_encrypt_row<FrP, W>(st0, k_cells, K, h_cells, H, p_cells, N, ct_cells, p_cells + T * 4, row + 4);
    }) ? ZL_OK : ZL_EINVAL;
}
// the same walk inside another circuit's rows (zl_poseidon_duplex_row_host): header and plaintext copied to their cells, the key read where the layout says
template <class FrP, int W>
int host_encrypt_rows_in(const uint64_t* init, const zl_duplex_row_layout& lay, size_t K, const uint64_t* headers, size_t H, const uint64_t* texts, size_t N, size_t count,
                         uint64_t* rows, size_t stride) {
    consts<FrP, W>();
    const size_t T = N * (W - 1);
    Fp<FrP> st0[W];
    for (int e = 0; e < W; e++) (void)load_canon<FrP>(init + 4 * e, st0[e]);
    return host_for(count, [&](size_t i) {
        uint64_t* row = rows + i * stride * 4;
        if (H) memcpy(row + lay.header * 4, headers + i * H * 4, H * 32);
        memcpy(row + lay.plain * 4, texts + i * T * 4, T * 32);
        return host_encrypt_row<FrP, W>(st0, row + lay.key * 4, K, row + lay.header * 4, H, row + lay.plain * 4, N, row + lay.ct * 4, row + lay.rec * 4, row + lay.tag * 4);
    }) ? ZL_OK : ZL_EINVAL;
}

// ---------------------------------------------------------------------------------------------------------------- device path: table, staging, launches
bool valid_curve(zl_curve_t c) { return c == ZL_BLS12_381 || c == ZL_BN254; }
size_t tune_chunk() {
    const int c = zl_tune("ZL_TUNE_POSEIDON_CHUNK", pd::DEFAULT_CHUNK);
    return c < 1 ? 1 : c > (1 << 24) ? (size_t)1 << 24 : (size_t)c;  // (a launch of 2^24 / 64 blocks at the most)
}
unsigned tune_tail() {
    const int t = zl_tune("ZL_TUNE_POSEIDON_TAIL", pd::DEFAULT_TAIL);
    return t < 0 ? 0u : t > pd::TAIL_MAX ? (unsigned)pd::TAIL_MAX : (unsigned)t;
}
bool on_host(const zl_ctx* ctx, size_t count) {
    if (!ctx) return true;
    const int m = zl_tune("ZL_TUNE_POSEIDON_DEV_MIN", pd::DEFAULT_DEV_MIN);
    return m > 0 && count < (size_t)m;
}
// staged items per chunk: the launch chunk, cut to the slot's byte budget
size_t stage_items(size_t bytes_per_item) {
    const size_t by_budget = pd::STAGE_BUDGET / bytes_per_item ? pd::STAGE_BUDGET / bytes_per_item : 1;
    const size_t c = tune_chunk();
    return c < by_budget ? c : by_budget;
}
constexpr size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
unsigned blocks_of(size_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

std::mutex& tab_mutex() {
    static std::mutex m;
    return m;
}
// The constant table of the (curve, width): built once by the first call for it on the ROOT ctx or any of its forks, owned by the root (zl_ctx_destroy frees
// it); the copy is synchronous, so the table is complete before the lock is released and any lane launches against it.
template <class FrP, int W = 3>
int get_table(zl_ctx* ctx, const uint32_t** out) {
    static_assert(sizeof(zl_ctx::poseidon_tab) / sizeof(void*) == 2 * pd::N_WIDTHS, "a slot per curve and width");
    constexpr pd::Spec S = pd::spec_of_width(W);
    zl_ctx* owner = ctx->parent ? ctx->parent : ctx;
    std::lock_guard<std::mutex> lk(tab_mutex());
    void*& slot = owner->poseidon_tab[(std::is_same<FrP, BLS12_381_Fr>::value ? 0 : pd::N_WIDTHS) + (W - pd::MIN_WIDTH)];
    if (!slot) {
        const poseidon::Constants<FrP, W>& c = consts<FrP, W>();
        std::vector<uint32_t> w((size_t)pd::tab_entries(W) * TABW, 0u);
        auto put = [&](int e, const Fp<FrP>& m) {
            const Fp<FrP> cw = zl::from_mont(m);
            const El<FrP> v = to_lazy<FrP>(cw.l);
            for (int k = 0; k < El<FrP>::L; k++) w[(size_t)e * TABW + k] = v.l[k];
        };
        for (int i = 0; i < (int)S.keys(); i++) put(pd::tab_keys(W) + i, c.round_keys[(size_t)i]);
        for (int i = 0; i < W; i++)
            for (int j = 0; j < W; j++) put(pd::tab_mds(W) + W * i + j, c.mds[i][j]);
        put(pd::tab_tag(W), zl::from_u64<FrP>(S.tag));
        void* d = nullptr;
        ZL_HIP(ctx, hipMalloc(&d, pd::tab_bytes(W)));
        const hipError_t e = hipMemcpy(d, w.data(), pd::tab_bytes(W), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            ctx->last_hip = (int)e;
            return ZL_EHIP;
        }
        slot = d;
    }
    *out = static_cast<const uint32_t*>(slot);
    return ZL_OK;
}
// the flag word (cleared) and `bytes` of staging behind it
struct Stage {
    uint32_t* flag = nullptr;
    unsigned char* data = nullptr;
};
int stage_get(zl_ctx* ctx, size_t bytes, Stage* s) {
    void* d = nullptr;
    const int rc = zl_scratch_get(ctx, ZL_SLOT_POSEIDON, pd::FLAG_BYTES + bytes, &d);
    if (rc) return rc;
    s->flag = static_cast<uint32_t*>(d);
    s->data = static_cast<unsigned char*>(d) + pd::FLAG_BYTES;
    ZL_HIP(ctx, hipMemsetAsync(s->flag, 0, 4, ctx->stream));
    return ZL_OK;
}
// wait for the call's work and read the flag: every entry point has finished when it returns
int finish(zl_ctx* ctx, const uint32_t* d_flag) {
    uint32_t bad = 0;
    ZL_HIP(ctx, hipMemcpyAsync(&bad, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    ZL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return bad ? ZL_EINVAL : ZL_OK;
}
#define ZL_POS_LAUNCH(ctx, kernel, grid, block, lds, ...)                          \
    do {                                                                           \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, (ctx)->stream, __VA_ARGS__); \
        ZL_HIP(ctx, hipGetLastError());                                            \
    } while (0)

// ---- the one staged-chunk runner: stage, chunk, upload, launch, download, finish.
// A staged segment of a call: `per` bytes per item, dense; item i of a chunk starting at `first` is up / down + (first + i) * per on the host.  per == 0: the
// segment is absent -- it takes no space and its device pointer is null, which is what the kernels' optional parameters (pub, tags, cts) expect.
struct Seg {
    size_t per;
    const void* up;  // host source, uploaded before the chunk's launch (may be null)
    void* down;      // host destination, downloaded behind it (may be null)
};
constexpr size_t MAX_SEGS = 6;
uint64_t* u64(void* p) { return static_cast<uint64_t*>(p); }
// Runs `count` items in chunks on ctx's stream and returns when they have finished (finish).  The chunk is the launch chunk, cut to the slot's byte budget by
// the bytes per item of the PRESENT segments (nothing staged: the launch chunk itself), so a chunk is never more than one launch.  Segment j lies at a 256-byte
// boundary of ONE stage_get; the flag word is cleared once, there, and read once, at the end.  Per chunk, in stream order: the uploads, then
// launch(first, m, d, flag) -- d[j] the device pointer of segment j, items first .. first + m - 1 of the call -- then the downloads.  A HIP error, or a non-zero
// return of `launch`, ends the call at that point.
// (Only present segments are charged.  The trace runners used to charge the 32 bytes of their optional public output whether it was asked for or not; without it
// a chunk may now be larger where the byte budget is the limit -- m0 * per <= STAGE_BUDGET holds as before.)
// Not through this runner: launch_merkle and the forest append (not this loop), and the two gathers dev_paths / dev_forest_paths, which raise no flag and end
// on a plain stream synchronise -- finish's read of the flag word cost them 20 us on calls of 33 - 54 us when they were tried here
// (profiles/poseidon_refactor_ab.log).
template <class Launch>
int run_chunks(zl_ctx* ctx, size_t count, std::initializer_list<Seg> segs, const Launch& launch) {
    if (segs.size() > MAX_SEGS) return ZL_EINVAL;
    size_t per = 0;
    for (const Seg& g : segs) per += g.per;
    const size_t chunk = per ? stage_items(per) : tune_chunk(), m0 = count < chunk ? count : chunk;
    size_t off[MAX_SEGS + 1] = {0}, ns = 0;
    for (const Seg& g : segs) {
        off[ns + 1] = off[ns] + up256(m0 * g.per);
        ns++;
    }
    Stage s;
    int rc = stage_get(ctx, off[ns], &s);
    if (rc) return rc;
    void* d[MAX_SEGS] = {};
    const Seg* sg = segs.begin();
    for (size_t j = 0; j < ns; j++) d[j] = sg[j].per ? s.data + off[j] : nullptr;
    for (size_t first = 0; first < count; first += chunk) {
        const size_t m = count - first < chunk ? count - first : chunk;
        for (size_t j = 0; j < ns; j++)
            if (sg[j].per && sg[j].up)
                ZL_HIP(ctx, hipMemcpyAsync(d[j], static_cast<const unsigned char*>(sg[j].up) + first * sg[j].per, m * sg[j].per, hipMemcpyHostToDevice, ctx->stream));
        if ((rc = launch(first, m, d, s.flag))) return rc;
        for (size_t j = 0; j < ns; j++)
            if (sg[j].per && sg[j].down)
                ZL_HIP(ctx, hipMemcpyAsync(static_cast<unsigned char*>(sg[j].down) + first * sg[j].per, d[j], m * sg[j].per, hipMemcpyDeviceToHost, ctx->stream));
    }
    return finish(ctx, s.flag);
}
// where a trace runner's chunk writes its rows: the staged segment (dense, nv elements apart) when the rows go to the host, else the caller's device rows
struct Rows {
    uint64_t* at;
    size_t stride;
};
Rows rows_of(void* d_staged, size_t nv, uint64_t* d_rows, size_t stride, size_t first) {
    return d_staged ? Rows{u64(d_staged), nv} : Rows{d_rows + first * stride * 4, stride};
}

// the batched permutation and hash at width W: W resp. W - 1 + 1 (inputs and digest) elements per item
template <class FrP, int W>
int dev_permute_w(zl_ctx* ctx, uint64_t* states, size_t count) {
    const uint32_t* tab;
    const int rc = get_table<FrP, W>(ctx, &tab);
    if (rc) return rc;
    return run_chunks(ctx, count, {{32 * W, states, states}}, [&](size_t, size_t m, void* const* d, uint32_t* flag) {
        ZL_POS_LAUNCH(ctx, (k_pos_permute_w<FrP, W>), blocks_of(m), BLOCK, 0, tab, u64(d[0]), m, flag);
        return ZL_OK;
    });
}
template <class FrP, int W>
int dev_hash_w_dev(zl_ctx* ctx, const void* d_in, size_t count, void* d_out) {
    const uint32_t* tab;
    const int rc = get_table<FrP, W>(ctx, &tab);
    if (rc) return rc;
    return run_chunks(ctx, count, {}, [&](size_t first, size_t m, void* const*, uint32_t* flag) {
        ZL_POS_LAUNCH(ctx, (k_pos_hash_w<FrP, W>), blocks_of(m), BLOCK, 0, tab, static_cast<const uint64_t*>(d_in) + first * (4 * (W - 1)), m,
                      static_cast<uint64_t*>(d_out) + first * 4, flag);
        return ZL_OK;
    });
}
template <class FrP, int W>
int dev_hash_w(zl_ctx* ctx, const uint64_t* in, size_t count, uint64_t* out) {
    const uint32_t* tab;
    const int rc = get_table<FrP, W>(ctx, &tab);
    if (rc) return rc;
    return run_chunks(ctx, count, {{32 * (W - 1), in, nullptr}, {32, nullptr, out}}, [&](size_t, size_t m, void* const* d, uint32_t* flag) {
        ZL_POS_LAUNCH(ctx, (k_pos_hash_w<FrP, W>), blocks_of(m), BLOCK, 0, tab, u64(d[0]), m, u64(d[1]), flag);
        return ZL_OK;
    });
}
template <class FrP>
int dev_chain(zl_ctx* ctx, const uint64_t* x0, const uint64_t* x1, uint32_t k, size_t count, uint64_t* out) {
    const uint32_t* tab;
    const int rc = get_table<FrP>(ctx, &tab);
    if (rc) return rc;
    return run_chunks(ctx, count, {{32, x0, nullptr}, {32, x1, nullptr}, {32, nullptr, out}}, [&](size_t, size_t m, void* const* d, uint32_t* flag) {
        ZL_POS_LAUNCH(ctx, (k_pos_chain<FrP>), blocks_of(m), BLOCK, 0, tab, u64(d[0]), u64(d[1]), k, m, u64(d[2]), flag);
        return ZL_OK;
    });
}
// Every form of the chain trace.  x0, x1: staged per chunk when in_on_host, else device memory; host_rows != null: the rows (nv = 4 + 234 k elements) are
// staged, dense, and downloaded (d_rows and stride are ignored), otherwise row i goes to d_rows + i * stride elements; host_pub != null: h_k of every chain is
// staged and downloaded.  A chunk is one launch.
template <class FrP>
int chain_trace_run(zl_ctx* ctx, const uint64_t* x0, const uint64_t* x1, bool in_on_host, uint32_t k, size_t count, uint64_t* d_rows, size_t stride, uint64_t* host_rows,
                    uint64_t* host_pub) {
    const uint32_t* tab;
    const int rc = get_table<FrP>(ctx, &tab);
    if (rc) return rc;
    const size_t nv = zl_poseidon_chain_assignment_elems(k), in_per = in_on_host ? 32 : 0;
    return run_chunks(ctx, count, {{in_per, x0, nullptr}, {in_per, x1, nullptr}, {host_rows ? nv * 32 : 0, nullptr, host_rows}, {host_pub ? 32u : 0u, nullptr, host_pub}},
                      [&](size_t first, size_t m, void* const* d, uint32_t* flag) {
                          const uint64_t* a = in_on_host ? u64(d[0]) : x0 + first * 4;
                          const uint64_t* b = in_on_host ? u64(d[1]) : x1 + first * 4;
                          const Rows rows = rows_of(d[2], nv, d_rows, stride, first);
                          ZL_POS_LAUNCH(ctx, (k_pos_chain_trace<FrP>), blocks_of(m), BLOCK, 0, tab, a, b, k, m, rows.at, rows.stride, u64(d[3]), flag);
                          return ZL_OK;
                      });
}
template <class FrP>
int dev_fold(zl_ctx* ctx, const uint64_t* leaves, const uint64_t* indices, const uint64_t* paths, unsigned depth, size_t count, uint64_t* roots) {
    const uint32_t* tab;
    const int rc = get_table<FrP>(ctx, &tab);
    if (rc) return rc;
    return run_chunks(ctx, count, {{32, leaves, nullptr}, {8, indices, nullptr}, {(size_t)depth * 32, paths, nullptr}, {32, nullptr, roots}},
                      [&](size_t, size_t m, void* const* d, uint32_t* flag) {
                          ZL_POS_LAUNCH(ctx, (k_pos_fold<FrP>), blocks_of(m), BLOCK, 0, tab, u64(d[0]), u64(d[1]), u64(d[2]), depth, m, u64(d[3]), flag);
                          return ZL_OK;
                      });
}
// every level of the tree in device memory (n >= 1): wide launches per level while a level has more than T nodes, then the one-workgroup tail
template <class FrP>
int launch_merkle(zl_ctx* ctx, const uint32_t* tab, const uint64_t* d_leaves, size_t n, unsigned depth, uint64_t* d_nodes, uint32_t* flag) {
    if (d_leaves != d_nodes) ZL_HIP(ctx, hipMemcpyAsync(d_nodes, d_leaves, n * 32, hipMemcpyDeviceToDevice, ctx->stream));
    const unsigned T = tune_tail();
    const size_t chunk = tune_chunk();
    size_t off = 0, cm = n;
    for (unsigned k = 1; k <= depth; k++) {
        uint64_t* child = d_nodes + off * 4;
        if (T && cm <= T) {
            const size_t lds = (cm + (cm + 1) / 2) * 32;
            ZL_POS_LAUNCH(ctx, (k_pos_tail<FrP>), 1, pd::TAIL_BLOCK, lds, tab, child, (unsigned)cm, depth - (k - 1), flag);
            break;
        }
        const size_t pm = (cm + 1) / 2;
        uint64_t* parent = child + cm * 4;
        for (size_t first = 0; first < pm; first += chunk) {
            const size_t m = pm - first < chunk ? pm - first : chunk;
            ZL_POS_LAUNCH(ctx, (k_pos_level<FrP>), blocks_of(m), BLOCK, 0, tab, child, cm, parent, first, m, flag);
        }
        off += cm;
        cm = pm;
    }
    return ZL_OK;
}
template <class FrP>
int dev_merkle_build_dev(zl_ctx* ctx, const void* d_leaves, size_t n, unsigned depth, void* d_nodes, uint64_t* root_out) {
    const uint32_t* tab;
    int rc = get_table<FrP>(ctx, &tab);
    if (rc) return rc;
    Stage s;
    if ((rc = stage_get(ctx, 0, &s))) return rc;
    uint64_t* nodes = static_cast<uint64_t*>(d_nodes);
    if ((rc = launch_merkle<FrP>(ctx, tab, static_cast<const uint64_t*>(d_leaves), n, depth, nodes, s.flag))) return rc;
    ZL_HIP(ctx, hipMemcpyAsync(root_out, nodes + (pd::level_offset(n, depth + 1) - 1) * 4, 32, hipMemcpyDeviceToHost, ctx->stream));
    return finish(ctx, s.flag);
}
struct DevFree {
    void operator()(void* p) const { (void)hipFree(p); }
};
// host leaves -> (optionally) the host node array and the root, through a node array of the call's own in device memory
template <class FrP>
int dev_merkle_host(zl_ctx* ctx, const uint64_t* leaves, size_t n, unsigned depth, uint64_t* nodes_out, uint64_t* root) {
    const size_t total = pd::level_offset(n, depth + 1);
    void* d = nullptr;
    ZL_HIP(ctx, hipMalloc(&d, total * 32));
    const std::unique_ptr<void, DevFree> hold(d);
    ZL_HIP(ctx, hipMemcpyAsync(d, leaves, n * 32, hipMemcpyHostToDevice, ctx->stream));
    int rc = dev_merkle_build_dev<FrP>(ctx, d, n, depth, d, root);
    if (rc == ZL_OK && nodes_out) {
        const hipError_t e = hipMemcpyAsync(nodes_out, d, total * 32, hipMemcpyDeviceToHost, ctx->stream);
        if (e != hipSuccess) { ctx->last_hip = (int)e; rc = ZL_EHIP; }
    }
    const hipError_t e = hipStreamSynchronize(ctx->stream);  // (also on the error paths: the block is freed behind this)
    if (e != hipSuccess && rc == ZL_OK) { ctx->last_hip = (int)e; rc = ZL_EHIP; }
    return rc;
}
LevelTable level_table(size_t n, unsigned depth) {
    LevelTable lt{};
    size_t off = 0;
    for (unsigned k = 0; k < depth; k++) {
        lt.off[k] = off;
        lt.size[k] = pd::level_size(n, k);
        off += lt.size[k];
    }
    return lt;
}
int dev_paths(zl_ctx* ctx, const void* d_nodes, size_t n, unsigned depth, const uint64_t* indices, size_t count, uint64_t* paths) {
    const size_t chunk = stage_items(8 + (size_t)depth * 32), m0 = count < chunk ? count : chunk, o_path = up256(m0 * 8);
    Stage s;
    const int rc = stage_get(ctx, o_path + m0 * depth * 32, &s);
    if (rc) return rc;
    uint64_t* d_idx = reinterpret_cast<uint64_t*>(s.data);
    uint64_t* d_path = reinterpret_cast<uint64_t*>(s.data + o_path);
    const LevelTable lt = level_table(n, depth);
    for (size_t first = 0; first < count; first += chunk) {
        const size_t m = count - first < chunk ? count - first : chunk;
        ZL_HIP(ctx, hipMemcpyAsync(d_idx, indices + first, m * 8, hipMemcpyHostToDevice, ctx->stream));
        ZL_POS_LAUNCH(ctx, k_pos_gather, blocks_of(m * depth), BLOCK, 0, static_cast<const uint64_t*>(d_nodes), lt, depth, d_idx, m * depth, d_path);
        ZL_HIP(ctx, hipMemcpyAsync(paths + first * depth * 4, d_path, m * depth * 32, hipMemcpyDeviceToHost, ctx->stream));
    }
    ZL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZL_OK;
}
// Every form of the membership trace.  Indices are host memory and are staged per chunk; a chunk is one launch (stage_items never exceeds the launch chunk).
//   hp != null: leaves and paths are HOST memory too and are staged beside the indices (Src is PathSrc and `src` is ignored);
//   host_rows != null: the rows are staged, dense, and downloaded (d_rows and stride are ignored), otherwise row i goes to d_rows + i * stride elements;
//   host_pub != null: the root of every item is staged and downloaded.
struct HostPaths {
    const uint64_t* leaves;
    const uint64_t* paths;
};
template <class FrP, class Src>
int merkle_trace_run(zl_ctx* ctx, Src src, const HostPaths* hp, const uint64_t* indices, unsigned depth, size_t count, uint64_t* d_rows, size_t stride, uint64_t* host_rows,
                     uint64_t* host_pub, const uint32_t* trees = nullptr) {
    const uint32_t* tab;
    const int rc = get_table<FrP>(ctx, &tab);
    if (rc) return rc;
    const size_t nv = pd::merkle_row_elems(depth);
    constexpr bool forest = std::is_same<Src, ForestSrc>::value;  // `trees` (host memory): the tree of every item, staged too
    return run_chunks(ctx, count,
                      {{8, indices, nullptr},
                       {hp ? 32u : 0u, hp ? hp->leaves : nullptr, nullptr},
                       {hp ? (size_t)depth * 32 : 0, hp ? hp->paths : nullptr, nullptr},
                       {forest ? 4u : 0u, trees, nullptr},
                       {host_rows ? nv * 32 : 0, nullptr, host_rows},
                       {host_pub ? 32u : 0u, nullptr, host_pub}},
                      [&](size_t first, size_t m, void* const* d, uint32_t* flag) {
                          Src from = src.advanced(first);
                          if constexpr (std::is_same<Src, PathSrc>::value) {
                              if (hp) from = PathSrc{u64(d[1]), u64(d[2]), depth};
                          }
                          if constexpr (forest) from.tree_of = static_cast<const uint32_t*>(d[3]);
                          const Rows rows = rows_of(d[4], nv, d_rows, stride, first);
                          ZL_POS_LAUNCH(ctx, (k_pos_merkle_trace<FrP, Src>), blocks_of(m), BLOCK, 0, tab, from, u64(d[0]), depth, m, rows.at, rows.stride, u64(d[5]), flag);
                          return ZL_OK;
                      });
}
template <class FrP>
int dev_merkle_from_host(zl_ctx* ctx, const uint64_t* leaves, const uint64_t* indices, const uint64_t* paths, unsigned depth, size_t count, uint64_t* d_rows, size_t stride,
                         uint64_t* host_rows, uint64_t* host_pub) {
    const HostPaths hp{leaves, paths};
    return merkle_trace_run<FrP, PathSrc>(ctx, PathSrc{nullptr, nullptr, depth}, &hp, indices, depth, count, d_rows, stride, host_rows, host_pub);
}
template <class FrP>
int dev_merkle_from_paths(zl_ctx* ctx, const void* d_leaves, const uint64_t* indices, const void* d_paths, unsigned depth, size_t count, void* d_rows, size_t stride) {
    const PathSrc src{static_cast<const uint64_t*>(d_leaves), static_cast<const uint64_t*>(d_paths), depth};
    return merkle_trace_run<FrP, PathSrc>(ctx, src, nullptr, indices, depth, count, static_cast<uint64_t*>(d_rows), stride, nullptr, nullptr);
}
template <class FrP>
int dev_merkle_from_tree(zl_ctx* ctx, const void* d_nodes, size_t n, unsigned depth, const uint64_t* indices, size_t count, void* d_rows, size_t stride, uint64_t* host_rows) {
    const TreeSrc src{static_cast<const uint64_t*>(d_nodes), level_table(n, depth)};
    return merkle_trace_run<FrP, TreeSrc>(ctx, src, nullptr, indices, depth, count, static_cast<uint64_t*>(d_rows), stride, host_rows, nullptr);
}
// Every form of the hash trace at width W.  in: count x (W - 1) elements, staged per chunk when in_on_host, else device memory; host_rows != null: the rows
// are staged, dense, and downloaded (d_rows and stride are ignored), otherwise row i goes to d_rows + i * stride elements; host_pub != null: the digest of
// every item is staged and downloaded.  A chunk is one launch.
template <class FrP, int W>
int hash_trace_run(zl_ctx* ctx, const uint64_t* in, bool in_on_host, size_t count, uint64_t* d_rows, size_t stride, uint64_t* host_rows, uint64_t* host_pub) {
    const uint32_t* tab;
    const int rc = get_table<FrP, W>(ctx, &tab);
    if (rc) return rc;
    constexpr size_t nv = pd::hash_row_elems(W - 1), in_per = 32 * (W - 1);
    return run_chunks(ctx, count, {{in_on_host ? in_per : 0, in, nullptr}, {host_rows ? nv * 32 : 0, nullptr, host_rows}, {host_pub ? 32u : 0u, nullptr, host_pub}},
                      [&](size_t first, size_t m, void* const* d, uint32_t* flag) {
                          const uint64_t* from = in_on_host ? u64(d[0]) : in + first * (4 * (W - 1));
                          const Rows rows = rows_of(d[1], nv, d_rows, stride, first);
                          ZL_POS_LAUNCH(ctx, (k_pos_hash_trace<FrP, W>), blocks_of(m), BLOCK, 0, tab, from, m, rows.at, rows.stride, u64(d[2]), flag);
                          return ZL_OK;
                      });
}
// Every form of the leaf-membership trace at width W, as merkle_trace_run: indices are host memory and staged per chunk; hp != null: preimages and paths
// are HOST memory and staged beside them (Src is LeafPathSrc and `src` is ignored); host_rows / host_pub as in hash_trace_run.
struct HostLeafPaths {
    const uint64_t* preimages;
    const uint64_t* paths;
};
template <class FrP, int W, class Src>
int leaf_trace_run(zl_ctx* ctx, Src src, const HostLeafPaths* hp, const uint64_t* indices, unsigned depth, size_t count, uint64_t* d_rows, size_t stride,
                   uint64_t* host_rows, uint64_t* host_pub) {
    const uint32_t *tab, *tab3;
    int rc = get_table<FrP, W>(ctx, &tab);
    if (rc || (rc = get_table<FrP>(ctx, &tab3))) return rc;
    const size_t nv = pd::leaf_row_elems(W - 1, depth);
    return run_chunks(ctx, count,
                      {{8, indices, nullptr},
                       {hp ? 32u * (W - 1) : 0u, hp ? hp->preimages : nullptr, nullptr},
                       {hp ? (size_t)depth * 32 : 0, hp ? hp->paths : nullptr, nullptr},
                       {host_rows ? nv * 32 : 0, nullptr, host_rows},
                       {host_pub ? 32u : 0u, nullptr, host_pub}},
                      [&](size_t first, size_t m, void* const* d, uint32_t* flag) {
                          Src from = src.advanced(first, W - 1);
                          if constexpr (std::is_same<Src, LeafPathSrc>::value) {
                              if (hp) from = LeafPathSrc{u64(d[1]), u64(d[2]), depth};
                          }
                          const Rows rows = rows_of(d[3], nv, d_rows, stride, first);
                          ZL_POS_LAUNCH(ctx, (k_pos_leaf_merkle_trace<FrP, W, Src>), blocks_of(m), BLOCK, 0, tab, tab3, from, u64(d[0]), depth, m, rows.at, rows.stride, u64(d[4]),
                                        flag);
                          return ZL_OK;
                      });
}
template <class FrP, int W>
int dev_leaf_from_host(zl_ctx* ctx, const uint64_t* preimages, const uint64_t* indices, const uint64_t* paths, unsigned depth, size_t count, uint64_t* d_rows, size_t stride,
                       uint64_t* host_rows, uint64_t* host_pub) {
    const HostLeafPaths hp{preimages, paths};
    return leaf_trace_run<FrP, W, LeafPathSrc>(ctx, LeafPathSrc{nullptr, nullptr, depth}, &hp, indices, depth, count, d_rows, stride, host_rows, host_pub);
}
template <class FrP, int W>
int dev_leaf_from_paths(zl_ctx* ctx, const void* d_preimages, const uint64_t* indices, const void* d_paths, unsigned depth, size_t count, void* d_rows, size_t stride) {
    const LeafPathSrc src{static_cast<const uint64_t*>(d_preimages), static_cast<const uint64_t*>(d_paths), depth};
    return leaf_trace_run<FrP, W, LeafPathSrc>(ctx, src, nullptr, indices, depth, count, static_cast<uint64_t*>(d_rows), stride, nullptr, nullptr);
}
template <class FrP, int W>
int dev_leaf_from_tree(zl_ctx* ctx, const void* d_nodes, const void* d_preimages, size_t n, unsigned depth, const uint64_t* indices, size_t count, void* d_rows,
                       size_t stride, uint64_t* host_rows) {
    const LeafTreeSrc src{static_cast<const uint64_t*>(d_nodes), static_cast<const uint64_t*>(d_preimages), level_table(n, depth)};
    return leaf_trace_run<FrP, W, LeafTreeSrc>(ctx, src, nullptr, indices, depth, count, static_cast<uint64_t*>(d_rows), stride, host_rows, nullptr);
}

// ---------------------------------------------------------------------------------------------------------------- the Merkle forest: host side
// What an append does, worked out on the host before anything is written: the slot of every leaf, the touched trees (in the order the input first names them)
// with their lengths before and after, and per level k = 1 .. depth the exclusive prefix sums of the trees' dirty ranges (row k - 1 of `pre`, T + 1 entries).
struct ForestPlan {
    std::vector<uint64_t> dst;
    std::vector<uint32_t> seg_tree;
    std::vector<uint64_t> seg_a, seg_b;
    std::vector<uint64_t> pre;
};
// ZL_EINVAL for a tree id >= trees or a tree that would grow past the capacity; the forest's lengths are not changed here (forest_commit)
int forest_plan(zl_merkle_forest* f, const uint32_t* tree_of, size_t count, ForestPlan& pl) {
    try {
        pl.dst.resize(count);
        bool ok = true;
        for (size_t i = 0; i < count && ok; i++) {
            const uint32_t t = tree_of[i];
            if (t >= f->trees) {
                ok = false;
                break;
            }
            if (f->add[t] == 0) pl.seg_tree.push_back(t);
            pl.dst[i] = (uint64_t)t * f->stride + f->lens[t] + f->add[t];
            f->add[t]++;
        }
        const size_t T = pl.seg_tree.size();
        pl.seg_a.resize(T);
        pl.seg_b.resize(T);
        for (size_t s = 0; s < T; s++) {
            const uint32_t t = pl.seg_tree[s];
            pl.seg_a[s] = f->lens[t];
            pl.seg_b[s] = f->lens[t] + f->add[t];
            if (pl.seg_b[s] > f->capacity) ok = false;
            f->add[t] = 0;
        }
        if (!ok) return ZL_EINVAL;
        pl.pre.resize((size_t)f->depth * (T + 1));
        for (unsigned k = 1; k <= f->depth; k++) {
            uint64_t* row = pl.pre.data() + (size_t)(k - 1) * (T + 1);
            row[0] = 0;
            for (size_t s = 0; s < T; s++) row[s + 1] = row[s] + (((pl.seg_b[s] - 1) >> k) - (pl.seg_a[s] >> k) + 1);
        }
    } catch (const std::bad_alloc&) {
        for (const uint32_t t : pl.seg_tree) f->add[t] = 0;
        return ZL_ENOMEM;
    }
    return ZL_OK;
}
void forest_commit(zl_merkle_forest* f, const ForestPlan& pl) {
    for (size_t s = 0; s < pl.seg_tree.size(); s++) f->lens[pl.seg_tree[s]] = pl.seg_b[s];
}
template <class FrP>
bool host_all_canon(const uint64_t* elems, size_t count) {
    for (size_t i = 0; i < count; i++)
        if (!canon_words<FrP>(elems + i * 4)) return false;
    return true;
}
// the host mirror's append: the leaves, then every level's dirty parents over the host pool -- the arithmetic of k_pos_forest_level through permute_native
template <class FrP>
int host_forest_append(zl_merkle_forest* f, const ForestPlan& pl, const uint64_t* leaves, size_t count) {
    consts<FrP>();
    for (size_t i = 0; i < count; i++) memcpy(f->nodes + pl.dst[i] * 4, leaves + i * 4, 32);
    const uint32_t T = (uint32_t)pl.seg_tree.size();
    bool ok = true;
    for (unsigned k = 1; k <= f->depth; k++) {
        const uint64_t* row = pl.pre.data() + (size_t)(k - 1) * (T + 1);
        const size_t child_off = pd::level_offset(f->capacity, k - 1), child_size = pd::level_size(f->capacity, k - 1), parent_off = child_off + child_size;
        ok &= host_for((size_t)row[T], [&](size_t q) {
            const uint32_t s = forest_seg(row, T, q);
            const size_t j = (size_t)(pl.seg_a[s] >> k) + (size_t)(q - row[s]);
            uint64_t* tree = f->nodes + (size_t)pl.seg_tree[s] * f->stride * 4;
            const uint64_t* child = tree + child_off * 4;
            return host_hash2<FrP>(child + 2 * j * 4, 2 * j + 1 < child_size ? child + (2 * j + 1) * 4 : nullptr, tree + (parent_off + j) * 4);
        });
    }
    return ok ? ZL_OK : ZL_EINVAL;
}
// The device append.  Staging (ZL_SLOT_POSEIDON): the touched-tree table and the prefix rows, uploaded once, then one chunk of leaves (host form) and their
// slots at a time.  Device leaves are validated in launches of their own, and the flag is read back, before the first node is written; host leaves were
// checked by the caller.  Every staged chunk is placed before level 1 is hashed; the launches of a level follow those of the level below on the stream.
template <class FrP>
int dev_forest_append(zl_merkle_forest* f, const ForestPlan& pl, const uint64_t* leaves, const uint64_t* d_leaves, size_t count) {
    zl_ctx* ctx = f->ctx;
    const uint32_t* tab;
    int rc = get_table<FrP>(ctx, &tab);
    if (rc) return rc;
    const size_t T = pl.seg_tree.size(), launch = tune_chunk();
    const size_t chunk = stage_items(leaves ? 40 : 8), m0 = count < chunk ? count : chunk;
    const size_t o_first = up256(T * 4), o_pre = o_first + up256(T * 8), o_leaf = o_pre + up256(pl.pre.size() * 8), o_dst = o_leaf + (leaves ? up256(m0 * 32) : 0);
    Stage s;
    if ((rc = stage_get(ctx, o_dst + m0 * 8, &s))) return rc;
    if (d_leaves) {
        for (size_t first = 0; first < count; first += launch) {
            const size_t m = count - first < launch ? count - first : launch;
            ZL_POS_LAUNCH(ctx, (k_pos_forest_place<FrP>), blocks_of(m), BLOCK, 0, d_leaves + first * 4, nullptr, m, nullptr, s.flag);
        }
        if ((rc = finish(ctx, s.flag))) return rc;  // (the flag word is still zero when this passes)
    }
    uint32_t* d_tree = reinterpret_cast<uint32_t*>(s.data);
    uint64_t* d_first = reinterpret_cast<uint64_t*>(s.data + o_first);
    uint64_t* d_pre = reinterpret_cast<uint64_t*>(s.data + o_pre);
    uint64_t* d_leaf = reinterpret_cast<uint64_t*>(s.data + o_leaf);
    uint64_t* d_dst = reinterpret_cast<uint64_t*>(s.data + o_dst);
    ZL_HIP(ctx, hipMemcpyAsync(d_tree, pl.seg_tree.data(), T * 4, hipMemcpyHostToDevice, ctx->stream));
    ZL_HIP(ctx, hipMemcpyAsync(d_first, pl.seg_a.data(), T * 8, hipMemcpyHostToDevice, ctx->stream));
    ZL_HIP(ctx, hipMemcpyAsync(d_pre, pl.pre.data(), pl.pre.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    for (size_t first = 0; first < count; first += chunk) {
        const size_t m = count - first < chunk ? count - first : chunk;
        if (leaves) ZL_HIP(ctx, hipMemcpyAsync(d_leaf, leaves + first * 4, m * 32, hipMemcpyHostToDevice, ctx->stream));
        ZL_HIP(ctx, hipMemcpyAsync(d_dst, pl.dst.data() + first, m * 8, hipMemcpyHostToDevice, ctx->stream));
        ZL_POS_LAUNCH(ctx, (k_pos_forest_place<FrP>), blocks_of(m), BLOCK, 0, leaves ? d_leaf : d_leaves + first * 4, d_dst, m, f->nodes, s.flag);
    }
    for (unsigned k = 1; k <= f->depth; k++) {
        const ForestSegs sg{d_tree, d_first, d_pre + (size_t)(k - 1) * (T + 1), (uint32_t)T};
        const size_t total = (size_t)pl.pre[(size_t)(k - 1) * (T + 1) + T];
        const size_t child_off = pd::level_offset(f->capacity, k - 1), child_size = pd::level_size(f->capacity, k - 1), parent_off = child_off + child_size;
        for (size_t first = 0; first < total; first += launch) {
            const size_t m = total - first < launch ? total - first : launch;
            ZL_POS_LAUNCH(ctx, (k_pos_forest_level<FrP>), blocks_of(m), BLOCK, 0, tab, f->nodes, f->stride, sg, k, child_off, child_size, parent_off, first, m, s.flag);
        }
    }
    return finish(ctx, s.flag);
}
// ZL_EINVAL unless every (tree, index) names a leaf the forest holds
int forest_members_ok(const zl_merkle_forest* f, const uint32_t* tree_of, const uint64_t* indices, size_t count) {
    for (size_t i = 0; i < count; i++)
        if (tree_of[i] >= f->trees || indices[i] >= f->lens[tree_of[i]]) return ZL_EINVAL;
    return ZL_OK;
}
int dev_forest_paths(const zl_merkle_forest* f, const uint32_t* tree_of, const uint64_t* indices, size_t count, uint64_t* paths) {
    zl_ctx* ctx = f->ctx;
    const unsigned depth = f->depth;
    const size_t chunk = stage_items(12 + (size_t)depth * 32), m0 = count < chunk ? count : chunk, o_tree = up256(m0 * 8), o_path = o_tree + up256(m0 * 4);
    Stage s;
    const int rc = stage_get(ctx, o_path + m0 * depth * 32, &s);
    if (rc) return rc;
    uint64_t* d_idx = reinterpret_cast<uint64_t*>(s.data);
    uint32_t* d_tree = reinterpret_cast<uint32_t*>(s.data + o_tree);
    uint64_t* d_path = reinterpret_cast<uint64_t*>(s.data + o_path);
    const LevelTable lt = level_table(f->capacity, depth);
    for (size_t first = 0; first < count; first += chunk) {
        const size_t m = count - first < chunk ? count - first : chunk;
        ZL_HIP(ctx, hipMemcpyAsync(d_idx, indices + first, m * 8, hipMemcpyHostToDevice, ctx->stream));
        ZL_HIP(ctx, hipMemcpyAsync(d_tree, tree_of + first, m * 4, hipMemcpyHostToDevice, ctx->stream));
        ZL_POS_LAUNCH(ctx, k_pos_forest_gather, blocks_of(m * depth), BLOCK, 0, f->nodes, f->stride, lt, depth, d_tree, d_idx, m * depth, d_path);
        ZL_HIP(ctx, hipMemcpyAsync(paths + first * depth * 4, d_path, m * depth * 32, hipMemcpyDeviceToHost, ctx->stream));
    }
    ZL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZL_OK;
}
// rows (and, host_pub != null, the root of every item) of memberships out of the forest, on `ctx`: the forest's own ctx or another lane of its device
template <class FrP>
int dev_merkle_from_forest(zl_ctx* ctx, const zl_merkle_forest* f, const uint32_t* tree_of, const uint64_t* indices, size_t count, void* d_rows, size_t stride,
                           uint64_t* host_rows, uint64_t* host_pub) {
    const ForestSrc src{f->nodes, f->stride, nullptr, level_table(f->capacity, f->depth)};
    return merkle_trace_run<FrP, ForestSrc>(ctx, src, nullptr, indices, f->depth, count, static_cast<uint64_t*>(d_rows), stride, host_rows, host_pub, tree_of);
}
// ---- the duplex cipher.  What a call is, beside its operands; init: W canonical elements, checked
struct DuplexCall {
    const uint64_t* init;
    size_t K, H, N;
    bool decrypt;
};
template <class FrP, int W>
int launch_duplex(zl_ctx* ctx, const uint32_t* tab, const DuplexCall& c, const uint64_t* d_keys, const uint64_t* d_headers, const uint64_t* d_in, size_t m, uint64_t* d_out,
                  uint64_t* d_tags, uint8_t* d_ok, uint32_t* flag) {
    DuplexInit init{};
    memcpy(init.w, c.init, 32 * W);
    ZL_POS_LAUNCH(ctx, (k_pos_duplex<FrP, W>), blocks_of(m), BLOCK, 0, tab, init, d_keys, (uint32_t)c.K, d_headers, (uint32_t)c.H, d_in, (uint32_t)c.N, m, d_out, d_tags, d_ok,
                  c.decrypt, flag);
    return ZL_OK;
}
// device operands, launches of at most one chunk; the verdicts of a decryption go through the staging area to ok_each (host memory)
template <class FrP, int W>
int dev_duplex_dev(zl_ctx* ctx, const DuplexCall& c, const void* d_keys, const void* d_headers, const void* d_in, size_t count, void* d_out, void* d_tags, uint8_t* ok_each) {
    const uint32_t* tab;
    const int rc = get_table<FrP, W>(ctx, &tab);
    if (rc) return rc;
    const size_t T = c.N * (W - 1);
    return run_chunks(ctx, count, {{c.decrypt ? 1u : 0u, nullptr, ok_each}}, [&](size_t first, size_t m, void* const* d, uint32_t* flag) {
        return launch_duplex<FrP, W>(ctx, tab, c, static_cast<const uint64_t*>(d_keys) + first * c.K * 4, static_cast<const uint64_t*>(d_headers) + first * c.H * 4,
                                     static_cast<const uint64_t*>(d_in) + first * T * 4, m, static_cast<uint64_t*>(d_out) + first * T * 4,
                                     static_cast<uint64_t*>(d_tags) + first * 4, static_cast<uint8_t*>(d[0]), flag);
    });
}
// host operands: keys, headers, texts (in place in the staging area), tags and verdicts of a chunk side by side
template <class FrP, int W>
int dev_duplex(zl_ctx* ctx, const DuplexCall& c, const uint64_t* keys, const uint64_t* headers, const uint64_t* text_in, size_t count, uint64_t* text_out, uint64_t* tags,
               uint8_t* ok_each) {
    const uint32_t* tab;
    const int rc = get_table<FrP, W>(ctx, &tab);
    if (rc) return rc;
    const size_t T = c.N * (W - 1);
    return run_chunks(ctx, count,
                      {{c.K * 32, keys, nullptr},
                       {c.H * 32, headers, nullptr},
                       {T * 32, text_in, text_out},
                       {32, c.decrypt ? tags : nullptr, c.decrypt ? nullptr : tags},
                       {1, nullptr, c.decrypt ? ok_each : nullptr}},
                      [&](size_t, size_t m, void* const* d, uint32_t* flag) {
                          return launch_duplex<FrP, W>(ctx, tab, c, u64(d[0]), u64(d[1]), u64(d[2]), m, u64(d[2]), u64(d[3]), static_cast<uint8_t*>(d[4]), flag);
                      });
}
// Every form of the encryption trace at width W (c.decrypt is unused).  keys / headers / texts: dense per item, staged per chunk when in_on_host, else device
// memory; host_rows != null: the rows are staged, dense, and downloaded (d_rows and stride are ignored), otherwise row i goes to d_rows + i * stride
// elements; host_tags / host_cts != null: the tag resp. the ciphertext of every item is staged and downloaded.  A chunk is one launch.
template <class FrP, int W>
int encrypt_trace_run(zl_ctx* ctx, const DuplexCall& c, const uint64_t* keys, const uint64_t* headers, const uint64_t* texts, bool in_on_host, size_t count, uint64_t* d_rows,
                      size_t stride, uint64_t* host_rows, uint64_t* host_tags, uint64_t* host_cts) {
    const uint32_t* tab;
    const int rc = get_table<FrP, W>(ctx, &tab);
    if (rc) return rc;
    const size_t T = c.N * (W - 1), nv = pd::encrypt_row_elems(W, c.K, c.H, c.N), in_elem = in_on_host ? 32 : 0;
    DuplexInit init{};
    memcpy(init.w, c.init, 32 * W);
    return run_chunks(ctx, count,
                      {{c.K * in_elem, keys, nullptr},
                       {c.H * in_elem, headers, nullptr},
                       {T * in_elem, texts, nullptr},
                       {host_rows ? nv * 32 : 0, nullptr, host_rows},
                       {host_tags ? 32u : 0u, nullptr, host_tags},
                       {host_cts ? T * 32 : 0, nullptr, host_cts}},
                      [&](size_t first, size_t m, void* const* d, uint32_t* flag) {
                          const uint64_t* k_from = in_on_host ? u64(d[0]) : keys + first * c.K * 4;
                          const uint64_t* h_from = in_on_host ? u64(d[1]) : headers + first * c.H * 4;
                          const uint64_t* t_from = in_on_host ? u64(d[2]) : texts + first * T * 4;
                          const Rows rows = rows_of(d[3], nv, d_rows, stride, first);
                          ZL_POS_LAUNCH(ctx, (k_pos_duplex_trace<FrP, W>), blocks_of(m), BLOCK, 0, tab, init, k_from, (uint32_t)c.K, h_from, (uint32_t)c.H, t_from, (uint32_t)c.N, m,
                                        rows.at, rows.stride, u64(d[4]), u64(d[5]), flag);
                          return ZL_OK;
                      });
}
// the parameters of a call: ZL_EINVAL, or ZL_OK with the initial state's words (zero for a null pointer) in init_out
template <class FrP>
bool duplex_init_ok(const uint64_t* w, unsigned width) {
    for (unsigned i = 0; i < width; i++)
        if (!canon_words<FrP>(w + 4 * i)) return false;
    return true;
}
int duplex_params(zl_curve_t curve, unsigned width, const uint64_t* initial_state, size_t key_len, size_t header_len, size_t blocks, uint64_t* init_out) {
    if (!valid_curve(curve) || zl_poseidon_duplex_permutations(width, key_len, header_len, blocks) == 0) return ZL_EINVAL;
    memset(init_out, 0, 32 * pd::MAX_WIDTH);
    if (initial_state) memcpy(init_out, initial_state, 32 * width);
    return (curve == ZL_BLS12_381 ? duplex_init_ok<BLS12_381_Fr>(init_out, width) : duplex_init_ok<BN254_Fr>(init_out, width)) ? ZL_OK : ZL_EINVAL;
}
}  // namespace

#define ZL_POS_CURVE(curve, fn, ...) ((curve) == ZL_BLS12_381 ? fn<BLS12_381_Fr>(__VA_ARGS__) : fn<BN254_Fr>(__VA_ARGS__))

int zl_poseidon_trace_rows(zl_ctx* ctx, int curve, const uint64_t* x0, const uint64_t* x1, uint32_t k, size_t count, void* d_rows, size_t stride_elems, uint64_t* public_out) {
    return ZL_POS_CURVE(curve, chain_trace_run, ctx, x0, x1, true, k, count, static_cast<uint64_t*>(d_rows), stride_elems, nullptr, public_out);
}
int zl_poseidon_merkle_trace_rows(zl_ctx* ctx, int curve, const uint64_t* leaves, const uint64_t* indices, const uint64_t* paths, unsigned depth, size_t count, void* d_rows,
                                  size_t stride_elems, uint64_t* roots_out) {
    return ZL_POS_CURVE(curve, dev_merkle_from_host, ctx, leaves, indices, paths, depth, count, static_cast<uint64_t*>(d_rows), stride_elems, nullptr, roots_out);
}
int zl_poseidon_merkle_member_rows(zl_ctx* ctx, int curve, const void* d_nodes, size_t n, unsigned depth, const uint64_t* indices, size_t count, void* d_rows,
                                   size_t stride_elems, uint64_t* host_rows) {
    return ZL_POS_CURVE(curve, dev_merkle_from_tree, ctx, d_nodes, n, depth, indices, count, d_rows, stride_elems, host_rows);
}
// every width of the table (3..6)
#define ZL_POS_ANYW_OF(FrP, width, fn, ...) \
    ((width) == 3 ? fn<FrP, 3>(__VA_ARGS__) : (width) == 4 ? fn<FrP, 4>(__VA_ARGS__) : (width) == 5 ? fn<FrP, 5>(__VA_ARGS__) : fn<FrP, 6>(__VA_ARGS__))
#define ZL_POS_ANYW(curve, width, fn, ...) \
    ((curve) == ZL_BLS12_381 ? ZL_POS_ANYW_OF(BLS12_381_Fr, width, fn, __VA_ARGS__) : ZL_POS_ANYW_OF(BN254_Fr, width, fn, __VA_ARGS__))
int zl_poseidon_hash_trace_rows(zl_ctx* ctx, int curve, unsigned arity, const uint64_t* in, size_t count, void* d_rows, size_t stride_elems, uint64_t* public_out) {
    return ZL_POS_ANYW(curve, arity + 1, hash_trace_run, ctx, in, true, count, static_cast<uint64_t*>(d_rows), stride_elems, nullptr, public_out);
}
int zl_poseidon_merkle_leaf_trace_rows(zl_ctx* ctx, int curve, unsigned arity, const uint64_t* preimages, const uint64_t* indices, const uint64_t* paths, unsigned depth,
                                       size_t count, void* d_rows, size_t stride_elems, uint64_t* roots_out) {
    return ZL_POS_ANYW(curve, arity + 1, dev_leaf_from_host, ctx, preimages, indices, paths, depth, count, static_cast<uint64_t*>(d_rows), stride_elems, nullptr, roots_out);
}
int zl_poseidon_merkle_leaf_member_rows(zl_ctx* ctx, int curve, unsigned arity, const void* d_nodes, const void* d_preimages, size_t n, unsigned depth,
                                        const uint64_t* indices, size_t count, void* d_rows, size_t stride_elems, uint64_t* host_rows) {
    return ZL_POS_ANYW(curve, arity + 1, dev_leaf_from_tree, ctx, d_nodes, d_preimages, n, depth, indices, count, d_rows, stride_elems, host_rows);
}
// one validation for every form of the encryption trace: the cipher's limits with key_len >= 1, the curve, the initial state (-> init_out, W elements)
static int encrypt_params(zl_curve_t curve, unsigned width, const uint64_t* initial_state, size_t key_len, size_t header_len, size_t blocks, uint64_t* init_out) {
    if (!pd::encrypt_shape_ok(width, key_len, header_len, blocks)) return ZL_EINVAL;
    return duplex_params(curve, width, initial_state, key_len, header_len, blocks, init_out);
}
int zl_poseidon_encrypt_trace_rows(zl_ctx* ctx, int curve, unsigned width, const uint64_t* initial_state, const uint64_t* keys, size_t key_len, const uint64_t* headers,
                                   size_t header_len, const uint64_t* plaintexts, size_t blocks, size_t count, void* d_rows, size_t stride_elems, uint64_t* tags_out,
                                   uint64_t* ciphertexts_out) {
    uint64_t init[4 * pd::MAX_WIDTH];
    const int rc = encrypt_params((zl_curve_t)curve, width, initial_state, key_len, header_len, blocks, init);
    if (rc) return rc;
    const DuplexCall c{init, key_len, header_len, blocks, false};
    return ZL_POS_ANYW(curve, width, encrypt_trace_run, ctx, c, keys, headers, plaintexts, true, count, static_cast<uint64_t*>(d_rows), stride_elems, nullptr, tags_out,
                       ciphertexts_out);
}
int zl_poseidon_duplex_row_params(int curve, unsigned width, const uint64_t* initial_state, size_t key_len, size_t header_len, size_t blocks, uint64_t* init_out) {
    return encrypt_params((zl_curve_t)curve, width, initial_state, key_len, header_len, blocks, init_out);
}
template <class FrP, int W>
static int duplex_row_launch(zl_ctx* ctx, const uint64_t* init_words, const zl_duplex_row_layout& lay, size_t K, const uint64_t* d_headers, size_t H, const uint64_t* d_texts,
                             size_t N, size_t m, uint64_t* d_rows, size_t stride, uint64_t* d_tags, uint64_t* d_cts, uint32_t* d_flag) {
    const uint32_t* tab;
    const int rc = get_table<FrP, W>(ctx, &tab);
    if (rc) return rc;
    DuplexInit init{};
    memcpy(init.w, init_words, 32 * W);
    ZL_POS_LAUNCH(ctx, (k_pos_duplex_trace_in<FrP, W>), blocks_of(m), BLOCK, 0, tab, init, lay, (uint32_t)K, d_headers, (uint32_t)H, d_texts, (uint32_t)N, m, d_rows, stride, d_tags,
                  d_cts, d_flag);
    return ZL_OK;
}
int zl_poseidon_duplex_row_launch(zl_ctx* ctx, int curve, unsigned width, const uint64_t* init, const zl_duplex_row_layout& lay, size_t key_len, const void* d_headers,
                                  size_t header_len, const void* d_plaintexts, size_t blocks, size_t m, void* d_rows, size_t stride_elems, void* d_tags, void* d_cts,
                                  uint32_t* d_flag) {
    return ZL_POS_ANYW(curve, width, duplex_row_launch, ctx, init, lay, key_len, static_cast<const uint64_t*>(d_headers), header_len, static_cast<const uint64_t*>(d_plaintexts),
                       blocks, m, static_cast<uint64_t*>(d_rows), stride_elems, static_cast<uint64_t*>(d_tags), static_cast<uint64_t*>(d_cts), d_flag);
}
int zl_poseidon_duplex_row_host(int curve, unsigned width, const uint64_t* init, const zl_duplex_row_layout& lay, size_t key_len, const uint64_t* headers, size_t header_len,
                                const uint64_t* plaintexts, size_t blocks, size_t count, uint64_t* rows, size_t stride_elems) {
    return ZL_POS_ANYW(curve, width, host_encrypt_rows_in, init, lay, key_len, headers, header_len, plaintexts, blocks, count, rows, stride_elems);
}

extern "C" {

// ---- every arity of the table (pd::spec); the width-3 / arity-2 entry points are these at width 3
int zl_poseidon_spec(unsigned arity, unsigned* width, unsigned* full_rounds, unsigned* partial_rounds, uint64_t* tag) {
    if (!pd::arity_ok(arity)) return ZL_EINVAL;
    const pd::Spec s = pd::spec(arity);
    if (width) *width = s.width;
    if (full_rounds) *full_rounds = s.full_rounds;
    if (partial_rounds) *partial_rounds = s.partial_rounds;
    if (tag) *tag = s.tag;
    return ZL_OK;
}
int zl_poseidon_permute_w(zl_curve_t curve, unsigned width, uint64_t* state) {
    if (!valid_curve(curve) || !pd::width_ok(width) || !state) return ZL_EINVAL;
    return ZL_POS_ANYW(curve, width, host_permute_one, state);
}
int zl_poseidon_constants(zl_curve_t curve, unsigned width, uint64_t* keys, uint64_t* mds) {
    if (!valid_curve(curve) || !pd::width_ok(width)) return ZL_EINVAL;
    return ZL_POS_ANYW(curve, width, constants_out, keys, mds);
}
int zl_poseidon_permute_batch_w(zl_ctx* ctx, zl_curve_t curve, unsigned width, uint64_t* states, size_t count) {
    if (!pd::width_ok(width) || !valid_curve(curve) || (count && !states)) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    if (on_host(ctx, count)) return ZL_POS_ANYW(curve, width, host_permute_w, states, count);
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_POS_ANYW(curve, width, dev_permute_w, ctx, states, count);
}
int zl_poseidon_hash_batch(zl_ctx* ctx, zl_curve_t curve, unsigned arity, const uint64_t* in, size_t count, uint64_t* out) {
    if (!pd::arity_ok(arity) || !valid_curve(curve) || (count && (!in || !out))) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    if (on_host(ctx, count)) return ZL_POS_ANYW(curve, arity + 1, host_hash_w, in, count, out);
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_POS_ANYW(curve, arity + 1, dev_hash_w, ctx, in, count, out);
}
int zl_poseidon_hash_batch_dev(zl_ctx* ctx, zl_curve_t curve, unsigned arity, const void* d_in, size_t count, void* d_out) {
    if (!pd::arity_ok(arity) || !ctx || !valid_curve(curve) || (count && (!d_in || !d_out))) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_POS_ANYW(curve, arity + 1, dev_hash_w_dev, ctx, d_in, count, d_out);
}
int zl_poseidon_permute_batch(zl_ctx* ctx, zl_curve_t curve, uint64_t* states, size_t count) { return zl_poseidon_permute_batch_w(ctx, curve, 3, states, count); }
int zl_poseidon_hash2_batch(zl_ctx* ctx, zl_curve_t curve, const uint64_t* xy, size_t count, uint64_t* out) { return zl_poseidon_hash_batch(ctx, curve, 2, xy, count, out); }
int zl_poseidon_hash2_batch_dev(zl_ctx* ctx, zl_curve_t curve, const void* d_xy, size_t count, void* d_out) {
    return zl_poseidon_hash_batch_dev(ctx, curve, 2, d_xy, count, d_out);
}
// ---- the duplex cipher: one validation (duplex_params), then the host mirror, the staged device path or the device-pointer path
size_t zl_poseidon_duplex_permutations(unsigned width, size_t key_len, size_t header_len, size_t blocks) {
    if (!pd::width_ok(width) || key_len > 64 || header_len > 64 || blocks < 1 || blocks > 1024) return 0;
    return poseidon::duplex_setup_blocks(width, key_len, header_len) + blocks;
}
static int duplex_batch(zl_ctx* ctx, zl_curve_t curve, unsigned width, const uint64_t* initial_state, const uint64_t* keys, size_t key_len, const uint64_t* headers,
                        size_t header_len, const uint64_t* text_in, size_t blocks, size_t count, uint64_t* text_out, uint64_t* tags, uint8_t* ok_each, bool decrypt) {
    uint64_t init[4 * pd::MAX_WIDTH];
    const int rc = duplex_params(curve, width, initial_state, key_len, header_len, blocks, init);
    if (rc) return rc;
    if (count && ((key_len && !keys) || (header_len && !headers) || !text_in || !text_out || !tags || (decrypt && !ok_each))) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    if (on_host(ctx, count)) return ZL_POS_ANYW(curve, width, host_duplex, init, keys, key_len, headers, header_len, text_in, blocks, count, text_out, tags, ok_each, decrypt);
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    const DuplexCall c{init, key_len, header_len, blocks, decrypt};
    return ZL_POS_ANYW(curve, width, dev_duplex, ctx, c, keys, headers, text_in, count, text_out, tags, ok_each);
}
static int duplex_batch_dev(zl_ctx* ctx, zl_curve_t curve, unsigned width, const uint64_t* initial_state, const void* d_keys, size_t key_len, const void* d_headers,
                            size_t header_len, const void* d_in, size_t blocks, size_t count, void* d_out, void* d_tags, uint8_t* ok_each, bool decrypt) {
    uint64_t init[4 * pd::MAX_WIDTH];
    const int rc = ctx ? duplex_params(curve, width, initial_state, key_len, header_len, blocks, init) : ZL_EINVAL;
    if (rc) return rc;
    if (count && ((key_len && !d_keys) || (header_len && !d_headers) || !d_in || !d_out || !d_tags || (decrypt && !ok_each))) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    const DuplexCall c{init, key_len, header_len, blocks, decrypt};
    return ZL_POS_ANYW(curve, width, dev_duplex_dev, ctx, c, d_keys, d_headers, d_in, count, d_out, d_tags, ok_each);
}
int zl_poseidon_duplex_encrypt_batch(zl_ctx* ctx, zl_curve_t curve, unsigned width, const uint64_t* initial_state, const uint64_t* keys, size_t key_len,
                                     const uint64_t* headers, size_t header_len, const uint64_t* plaintexts, size_t blocks, size_t count, uint64_t* ciphertexts,
                                     uint64_t* tags) {
    return duplex_batch(ctx, curve, width, initial_state, keys, key_len, headers, header_len, plaintexts, blocks, count, ciphertexts, tags, nullptr, false);
}
int zl_poseidon_duplex_decrypt_batch(zl_ctx* ctx, zl_curve_t curve, unsigned width, const uint64_t* initial_state, const uint64_t* keys, size_t key_len,
                                     const uint64_t* headers, size_t header_len, const uint64_t* ciphertexts, const uint64_t* tags, size_t blocks, size_t count,
                                     uint64_t* plaintexts, uint8_t* ok_each) {
    return duplex_batch(ctx, curve, width, initial_state, keys, key_len, headers, header_len, ciphertexts, blocks, count, plaintexts, const_cast<uint64_t*>(tags), ok_each,
                        true);  // (tags is only read when decrypting)
}
int zl_poseidon_duplex_encrypt_batch_dev(zl_ctx* ctx, zl_curve_t curve, unsigned width, const uint64_t* initial_state, const void* d_keys, size_t key_len,
                                         const void* d_headers, size_t header_len, const void* d_plaintexts, size_t blocks, size_t count, void* d_ciphertexts,
                                         void* d_tags) {
    return duplex_batch_dev(ctx, curve, width, initial_state, d_keys, key_len, d_headers, header_len, d_plaintexts, blocks, count, d_ciphertexts, d_tags, nullptr, false);
}
int zl_poseidon_duplex_decrypt_batch_dev(zl_ctx* ctx, zl_curve_t curve, unsigned width, const uint64_t* initial_state, const void* d_keys, size_t key_len,
                                         const void* d_headers, size_t header_len, const void* d_ciphertexts, const void* d_tags, size_t blocks, size_t count,
                                         void* d_plaintexts, uint8_t* ok_each) {
    return duplex_batch_dev(ctx, curve, width, initial_state, d_keys, key_len, d_headers, header_len, d_ciphertexts, blocks, count, d_plaintexts, const_cast<void*>(d_tags),
                            ok_each, true);
}
// ---- the encryption circuit's assignments: the cipher's validation plus the circuit's (encrypt_params), then the host mirror or the trace kernel
size_t zl_poseidon_encrypt_assignment_elems(unsigned width, size_t key_len, size_t header_len, size_t blocks) {
    return pd::encrypt_shape_ok(width, key_len, header_len, blocks) ? pd::encrypt_row_elems(width, key_len, header_len, blocks) : 0;
}
int zl_poseidon_encrypt_assignments(zl_ctx* ctx, zl_curve_t curve, unsigned width, const uint64_t* initial_state, const uint64_t* keys, size_t key_len,
                                    const uint64_t* headers, size_t header_len, const uint64_t* plaintexts, size_t blocks, size_t count, uint64_t* out) {
    uint64_t init[4 * pd::MAX_WIDTH];
    const int rc = encrypt_params(curve, width, initial_state, key_len, header_len, blocks, init);
    if (rc) return rc;
    const size_t nv = pd::encrypt_row_elems(width, key_len, header_len, blocks);  // (with its inputs within the staging budget at every shape: zl_poseidon_dev.h)
    if (count && (!keys || (header_len && !headers) || !plaintexts || !out)) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    if (on_host(ctx, count)) return ZL_POS_ANYW(curve, width, host_encrypt_assignments, init, keys, key_len, headers, header_len, plaintexts, blocks, count, out, nv);
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    const DuplexCall c{init, key_len, header_len, blocks, false};
    return ZL_POS_ANYW(curve, width, encrypt_trace_run, ctx, c, keys, headers, plaintexts, true, count, nullptr, 0, out, nullptr, nullptr);
}
int zl_poseidon_encrypt_assignments_dev(zl_ctx* ctx, zl_curve_t curve, unsigned width, const uint64_t* initial_state, const void* d_keys, size_t key_len,
                                        const void* d_headers, size_t header_len, const void* d_plaintexts, size_t blocks, size_t count, void* d_out, size_t stride_elems) {
    uint64_t init[4 * pd::MAX_WIDTH];
    const int rc = ctx ? encrypt_params(curve, width, initial_state, key_len, header_len, blocks, init) : ZL_EINVAL;
    if (rc) return rc;
    if (stride_elems < pd::encrypt_row_elems(width, key_len, header_len, blocks) || ((uintptr_t)d_out & 15)) return ZL_EINVAL;
    if (count && (!d_keys || (header_len && !d_headers) || !d_plaintexts || !d_out)) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    const DuplexCall c{init, key_len, header_len, blocks, false};
    return ZL_POS_ANYW(curve, width, encrypt_trace_run, ctx, c, static_cast<const uint64_t*>(d_keys), static_cast<const uint64_t*>(d_headers),
                       static_cast<const uint64_t*>(d_plaintexts), false, count, static_cast<uint64_t*>(d_out), stride_elems, nullptr, nullptr, nullptr);
}
int zl_poseidon_chain_batch(zl_ctx* ctx, zl_curve_t curve, const uint64_t* x0, const uint64_t* x1, uint32_t k, size_t count, uint64_t* out) {
    if (!valid_curve(curve) || k == 0 || (count && (!x0 || !x1 || !out))) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    if (on_host(ctx, count)) return ZL_POS_CURVE(curve, host_chain, x0, x1, k, count, out);
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_POS_CURVE(curve, dev_chain, ctx, x0, x1, k, count, out);
}
size_t zl_poseidon_chain_assignment_elems(uint32_t k) {
    const uint64_t nv = 4 + (uint64_t)pd::TRACE_PER_LINK * k;
    return k == 0 || nv >= (1ull << 31) ? 0 : (size_t)nv;
}
int zl_poseidon_chain_assignments_dev(zl_ctx* ctx, zl_curve_t curve, const void* d_x0, const void* d_x1, uint32_t k, size_t count, void* d_out, size_t stride_elems) {
    const size_t nv = zl_poseidon_chain_assignment_elems(k);
    if (!ctx || !valid_curve(curve) || nv == 0 || stride_elems < nv || (count && (!d_x0 || !d_x1 || !d_out)) || ((uintptr_t)d_out & 15)) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_POS_CURVE(curve, chain_trace_run, ctx, static_cast<const uint64_t*>(d_x0), static_cast<const uint64_t*>(d_x1), false, k, count, static_cast<uint64_t*>(d_out),
                        stride_elems, nullptr, nullptr);
}
int zl_poseidon_chain_assignments(zl_ctx* ctx, zl_curve_t curve, const uint64_t* x0, const uint64_t* x1, uint32_t k, size_t count, uint64_t* out) {
    const size_t nv = zl_poseidon_chain_assignment_elems(k);
    // (a staged chunk holds whole rows: one row with its inputs must fit the slot's byte budget, k <= 35 848)
    if (!valid_curve(curve) || nv == 0 || 64 + nv * 32 > pd::STAGE_BUDGET || (count && (!x0 || !x1 || !out))) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    if (on_host(ctx, count)) return ZL_POS_CURVE(curve, host_assignments, x0, x1, k, count, out, nv);
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_POS_CURVE(curve, chain_trace_run, ctx, x0, x1, true, k, count, nullptr, 0, out, nullptr);
}
size_t zl_poseidon_merkle_nodes(size_t n, unsigned depth) {
    return pd::geometry_ok(n, depth) ? pd::level_offset(n, depth + 1) : 0;
}
int zl_poseidon_merkle_build_dev(zl_ctx* ctx, zl_curve_t curve, const void* d_leaves, size_t n, unsigned depth, void* d_nodes, uint64_t* root_out) {
    if (!ctx || !valid_curve(curve) || !pd::geometry_ok(n, depth) || !root_out || (n && (!d_leaves || !d_nodes))) return ZL_EINVAL;
    if (n == 0) {
        memset(root_out, 0, 32);
        return ZL_OK;
    }
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_POS_CURVE(curve, dev_merkle_build_dev, ctx, d_leaves, n, depth, d_nodes, root_out);
}
int zl_poseidon_merkle_build(zl_ctx* ctx, zl_curve_t curve, const uint64_t* leaves, size_t n, unsigned depth, uint64_t* nodes, uint64_t* root) {
    if (!valid_curve(curve) || !pd::geometry_ok(n, depth) || !root || (n && (!leaves || !nodes))) return ZL_EINVAL;
    if (n == 0) {
        memset(root, 0, 32);
        return ZL_OK;
    }
    if (on_host(ctx, n)) {
        const int rc = ZL_POS_CURVE(curve, host_merkle, leaves, n, depth, nodes);
        memcpy(root, nodes + (pd::level_offset(n, depth + 1) - 1) * 4, 32);
        return rc;
    }
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_POS_CURVE(curve, dev_merkle_host, ctx, leaves, n, depth, nodes, root);
}
int zl_poseidon_merkle_root(zl_ctx* ctx, zl_curve_t curve, const uint64_t* leaves, size_t n, unsigned depth, uint64_t* root) {
    if (!valid_curve(curve) || !pd::geometry_ok(n, depth) || !root || (n && !leaves)) return ZL_EINVAL;
    if (n == 0) {
        memset(root, 0, 32);
        return ZL_OK;
    }
    if (on_host(ctx, n)) {
        const size_t total = pd::level_offset(n, depth + 1);
        const std::unique_ptr<uint64_t[]> nodes(new (std::nothrow) uint64_t[total * 4]);
        if (!nodes) return ZL_ENOMEM;
        const int rc = ZL_POS_CURVE(curve, host_merkle, leaves, n, depth, nodes.get());
        memcpy(root, nodes.get() + (total - 1) * 4, 32);
        return rc;
    }
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_POS_CURVE(curve, dev_merkle_host, ctx, leaves, n, depth, nullptr, root);
}
static int paths_args_ok(size_t n, unsigned depth, const uint64_t* indices, size_t count, const uint64_t* paths) {
    if (!pd::geometry_ok(n, depth) || (count && (!indices || !paths))) return 0;
    for (size_t i = 0; i < count; i++)
        if (indices[i] >= n) return 0;
    return 1;
}
int zl_poseidon_merkle_paths_dev(zl_ctx* ctx, zl_curve_t curve, const void* d_nodes, size_t n, unsigned depth, const uint64_t* indices, size_t count,
                                 uint64_t* paths) {
    if (!ctx || !valid_curve(curve) || !paths_args_ok(n, depth, indices, count, paths) || (count && !d_nodes)) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return dev_paths(ctx, d_nodes, n, depth, indices, count, paths);
}
int zl_poseidon_merkle_paths(const uint64_t* nodes, size_t n, unsigned depth, const uint64_t* indices, size_t count, uint64_t* paths) {
    if (!paths_args_ok(n, depth, indices, count, paths) || (count && !nodes)) return ZL_EINVAL;
    const LevelTable lt = level_table(n, depth);
    for (size_t i = 0; i < count; i++)
        for (unsigned k = 0; k < depth; k++) {
            const uint64_t sib = (indices[i] >> k) ^ 1;
            uint64_t* dst = paths + (i * depth + k) * 4;
            if (sib < lt.size[k]) memcpy(dst, nodes + (lt.off[k] + sib) * 4, 32);
            else memset(dst, 0, 32);
        }
    return ZL_OK;
}
int zl_poseidon_merkle_roots_from_paths(zl_ctx* ctx, zl_curve_t curve, const uint64_t* leaves, const uint64_t* indices, const uint64_t* paths, unsigned depth,
                                        size_t count, uint64_t* roots) {
    if (!valid_curve(curve) || depth < 1 || depth > pd::MAX_DEPTH || (count && (!leaves || !indices || !paths || !roots))) return ZL_EINVAL;
    for (size_t i = 0; i < count; i++)
        if (indices[i] >> depth) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    if (on_host(ctx, count)) return ZL_POS_CURVE(curve, host_fold, leaves, indices, paths, depth, count, roots);
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_POS_CURVE(curve, dev_fold, ctx, leaves, indices, paths, depth, count, roots);
}
size_t zl_poseidon_merkle_assignment_elems(unsigned depth) {
    return depth < 1 || depth > pd::MAX_DEPTH ? 0 : pd::merkle_row_elems(depth);
}
static int indices_below(const uint64_t* indices, size_t count, uint64_t bound) {
    for (size_t i = 0; i < count; i++)
        if (indices[i] >= bound) return 0;
    return 1;
}
int zl_poseidon_merkle_assignments(zl_ctx* ctx, zl_curve_t curve, const uint64_t* leaves, const uint64_t* indices, const uint64_t* paths, unsigned depth, size_t count,
                                   uint64_t* out) {
    const size_t nv = zl_poseidon_merkle_assignment_elems(depth);
    if (!valid_curve(curve) || nv == 0 || (count && (!leaves || !indices || !paths || !out)) || !indices_below(indices, count, (uint64_t)1 << depth)) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    if (on_host(ctx, count)) return ZL_POS_CURVE(curve, host_merkle_assignments, leaves, indices, paths, depth, count, out, nv);
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_POS_CURVE(curve, dev_merkle_from_host, ctx, leaves, indices, paths, depth, count, nullptr, nv, out, nullptr);
}
int zl_poseidon_merkle_assignments_dev(zl_ctx* ctx, zl_curve_t curve, const void* d_leaves, const uint64_t* indices, const void* d_paths, unsigned depth, size_t count,
                                       void* d_out, size_t stride_elems) {
    const size_t nv = zl_poseidon_merkle_assignment_elems(depth);
    if (!ctx || !valid_curve(curve) || nv == 0 || stride_elems < nv || (count && (!d_leaves || !indices || !d_paths || !d_out)) || ((uintptr_t)d_out & 15) ||
        !indices_below(indices, count, (uint64_t)1 << depth))
        return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_POS_CURVE(curve, dev_merkle_from_paths, ctx, d_leaves, indices, d_paths, depth, count, d_out, stride_elems);
}
int zl_poseidon_merkle_member_assignments_dev(zl_ctx* ctx, zl_curve_t curve, const void* d_nodes, size_t n, unsigned depth, const uint64_t* indices, size_t count,
                                              void* d_out, size_t stride_elems) {
    const size_t nv = zl_poseidon_merkle_assignment_elems(depth);
    if (!ctx || !valid_curve(curve) || nv == 0 || !pd::geometry_ok(n, depth) || stride_elems < nv || (count && (!d_nodes || !indices || !d_out)) ||
        ((uintptr_t)d_out & 15) || !indices_below(indices, count, n))
        return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_POS_CURVE(curve, dev_merkle_from_tree, ctx, d_nodes, n, depth, indices, count, d_out, stride_elems, nullptr);
}
// ---- the assignments of the arity-general circuits (zl_circuit_poseidon_hash, zl_circuit_poseidon_merkle_leaf)
size_t zl_poseidon_hash_assignment_elems(unsigned arity) {
    return pd::arity_ok(arity) ? pd::hash_row_elems(arity) : 0;
}
size_t zl_poseidon_merkle_leaf_assignment_elems(unsigned arity, unsigned depth) {
    return !pd::arity_ok(arity) || depth < 1 || depth > pd::MAX_DEPTH ? 0 : pd::leaf_row_elems(arity, depth);
}
int zl_poseidon_hash_assignments(zl_ctx* ctx, zl_curve_t curve, unsigned arity, const uint64_t* in, size_t count, uint64_t* out) {
    if (!valid_curve(curve) || !pd::arity_ok(arity) || (count && (!in || !out))) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    if (on_host(ctx, count)) return ZL_POS_ANYW(curve, arity + 1, host_hash_assignments, in, count, out);
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_POS_ANYW(curve, arity + 1, hash_trace_run, ctx, in, true, count, nullptr, 0, out, nullptr);
}
int zl_poseidon_hash_assignments_dev(zl_ctx* ctx, zl_curve_t curve, unsigned arity, const void* d_in, size_t count, void* d_out, size_t stride_elems) {
    const size_t nv = zl_poseidon_hash_assignment_elems(arity);
    if (!ctx || !valid_curve(curve) || nv == 0 || stride_elems < nv || (count && (!d_in || !d_out)) || ((uintptr_t)d_out & 15)) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_POS_ANYW(curve, arity + 1, hash_trace_run, ctx, static_cast<const uint64_t*>(d_in), false, count, static_cast<uint64_t*>(d_out), stride_elems, nullptr, nullptr);
}
int zl_poseidon_merkle_leaf_assignments(zl_ctx* ctx, zl_curve_t curve, unsigned arity, const uint64_t* preimages, const uint64_t* indices, const uint64_t* paths,
                                        unsigned depth, size_t count, uint64_t* out) {
    const size_t nv = zl_poseidon_merkle_leaf_assignment_elems(arity, depth);
    if (!valid_curve(curve) || nv == 0 || (count && (!preimages || !indices || !paths || !out)) || !indices_below(indices, count, (uint64_t)1 << depth)) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    if (on_host(ctx, count)) return ZL_POS_ANYW(curve, arity + 1, host_leaf_assignments, preimages, indices, paths, depth, count, out);
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_POS_ANYW(curve, arity + 1, dev_leaf_from_host, ctx, preimages, indices, paths, depth, count, nullptr, nv, out, nullptr);
}
int zl_poseidon_merkle_leaf_assignments_dev(zl_ctx* ctx, zl_curve_t curve, unsigned arity, const void* d_preimages, const uint64_t* indices, const void* d_paths,
                                            unsigned depth, size_t count, void* d_out, size_t stride_elems) {
    const size_t nv = zl_poseidon_merkle_leaf_assignment_elems(arity, depth);
    if (!ctx || !valid_curve(curve) || nv == 0 || stride_elems < nv || (count && (!d_preimages || !indices || !d_paths || !d_out)) || ((uintptr_t)d_out & 15) ||
        !indices_below(indices, count, (uint64_t)1 << depth))
        return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_POS_ANYW(curve, arity + 1, dev_leaf_from_paths, ctx, d_preimages, indices, d_paths, depth, count, d_out, stride_elems);
}
int zl_poseidon_merkle_leaf_member_assignments_dev(zl_ctx* ctx, zl_curve_t curve, unsigned arity, const void* d_nodes, const void* d_preimages, size_t n, unsigned depth,
                                                   const uint64_t* indices, size_t count, void* d_out, size_t stride_elems) {
    const size_t nv = zl_poseidon_merkle_leaf_assignment_elems(arity, depth);
    if (!ctx || !valid_curve(curve) || nv == 0 || !pd::geometry_ok(n, depth) || stride_elems < nv || (count && (!d_nodes || !d_preimages || !indices || !d_out)) ||
        ((uintptr_t)d_out & 15) || !indices_below(indices, count, n))
        return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_POS_ANYW(curve, arity + 1, dev_leaf_from_tree, ctx, d_nodes, d_preimages, n, depth, indices, count, d_out, stride_elems, nullptr);
}

// ---- the Merkle forest
int zl_merkle_forest_create(zl_ctx* ctx, zl_curve_t curve, uint32_t trees, unsigned depth, size_t capacity, zl_merkle_forest** out) {
    if (!out) return ZL_EINVAL;
    *out = nullptr;
    if (!valid_curve(curve) || trees < 1 || trees > 65536 || capacity < 1 || !pd::geometry_ok(capacity, depth)) return ZL_EINVAL;
    std::unique_ptr<zl_merkle_forest> f(new (std::nothrow) zl_merkle_forest);
    if (!f) return ZL_ENOMEM;
    f->ctx = ctx;
    f->curve = curve;
    f->trees = trees;
    f->depth = depth;
    f->capacity = capacity;
    f->stride = pd::level_offset(capacity, depth + 1);
    try {
        f->lens.assign(trees, 0);
        f->add.assign(trees, 0);
    } catch (const std::bad_alloc&) {
        return ZL_ENOMEM;
    }
    if (f->stride > (SIZE_MAX >> 5) / trees) return ZL_ENOMEM;
    const size_t bytes = (size_t)trees * f->stride * 32;
    if (!ctx) {
        f->nodes = static_cast<uint64_t*>(calloc(bytes, 1));
        if (!f->nodes) return ZL_ENOMEM;
    } else {
        ZL_HIP(ctx, hipSetDevice(ctx->device));
        void* d = nullptr;
        const hipError_t e = hipMalloc(&d, bytes);
        if (e != hipSuccess) {
            ctx->last_hip = (int)e;
            return ZL_ENOMEM;
        }
        std::unique_ptr<void, DevFree> hold(d);  // (freed on the error returns below)
        ZL_HIP(ctx, hipMemsetAsync(d, 0, bytes, ctx->stream));
        ZL_HIP(ctx, hipStreamSynchronize(ctx->stream));
        f->nodes = static_cast<uint64_t*>(hold.release());
    }
    *out = f.release();
    return ZL_OK;
}
void zl_merkle_forest_destroy(zl_merkle_forest* f) {
    if (!f) return;
    if (!f->ctx) {
        free(f->nodes);
    } else {
        (void)hipSetDevice(f->ctx->device);
        (void)hipFree(f->nodes);  // (every call on the forest had finished when it returned; hipFree waits for the device besides)
    }
    delete f;
}
int zl_merkle_forest_describe(const zl_merkle_forest* f, uint32_t* trees, unsigned* depth, size_t* capacity, size_t* tree_stride_elems) {
    if (!f) return ZL_EINVAL;
    if (trees) *trees = f->trees;
    if (depth) *depth = f->depth;
    if (capacity) *capacity = f->capacity;
    if (tree_stride_elems) *tree_stride_elems = f->stride;
    return ZL_OK;
}
int zl_merkle_forest_lens(const zl_merkle_forest* f, uint64_t* lens) {
    if (!f || !lens) return ZL_EINVAL;
    memcpy(lens, f->lens.data(), (size_t)f->trees * 8);
    return ZL_OK;
}
int zl_merkle_forest_append(zl_merkle_forest* f, const uint32_t* tree_of, const uint64_t* leaves, size_t count) {
    if (!f || (count && (!tree_of || !leaves))) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    if (!ZL_POS_CURVE(f->curve, host_all_canon, leaves, count)) return ZL_EINVAL;
    ForestPlan pl;
    int rc = forest_plan(f, tree_of, count, pl);
    if (rc) return rc;
    if (!f->ctx) {
        rc = ZL_POS_CURVE(f->curve, host_forest_append, f, pl, leaves, count);
    } else {
        ZL_HIP(f->ctx, hipSetDevice(f->ctx->device));
        rc = ZL_POS_CURVE(f->curve, dev_forest_append, f, pl, leaves, nullptr, count);
    }
    if (rc == ZL_OK) forest_commit(f, pl);
    return rc;
}
int zl_merkle_forest_append_dev(zl_merkle_forest* f, const uint32_t* tree_of, const void* d_leaves, size_t count) {
    if (!f || !f->ctx || (count && (!tree_of || !d_leaves))) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    ForestPlan pl;
    int rc = forest_plan(f, tree_of, count, pl);
    if (rc) return rc;
    ZL_HIP(f->ctx, hipSetDevice(f->ctx->device));
    rc = ZL_POS_CURVE(f->curve, dev_forest_append, f, pl, nullptr, static_cast<const uint64_t*>(d_leaves), count);
    if (rc == ZL_OK) forest_commit(f, pl);
    return rc;
}
int zl_merkle_forest_roots(const zl_merkle_forest* f, uint64_t* roots) {
    if (!f || !roots) return ZL_EINVAL;
    const uint64_t* first = f->nodes + (f->stride - 1) * 4;  // the root is a tree's last node
    if (!f->ctx) {
        for (uint32_t t = 0; t < f->trees; t++) memcpy(roots + (size_t)t * 4, first + (size_t)t * f->stride * 4, 32);
        return ZL_OK;
    }
    zl_ctx* ctx = f->ctx;
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    ZL_HIP(ctx, hipMemcpy2DAsync(roots, 32, first, f->stride * 32, 32, f->trees, hipMemcpyDeviceToHost, ctx->stream));  // one strided copy, no kernel
    ZL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZL_OK;
}
int zl_merkle_forest_paths(const zl_merkle_forest* f, const uint32_t* tree_of, const uint64_t* indices, size_t count, uint64_t* paths) {
    if (!f || (count && (!tree_of || !indices || !paths)) || forest_members_ok(f, tree_of, indices, count)) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    if (!f->ctx) {
        for (size_t i = 0; i < count; i++) {
            const int rc = zl_poseidon_merkle_paths(f->nodes + (size_t)tree_of[i] * f->stride * 4, f->capacity, f->depth, indices + i, 1, paths + i * f->depth * 4);
            if (rc) return rc;
        }
        return ZL_OK;
    }
    ZL_HIP(f->ctx, hipSetDevice(f->ctx->device));
    return dev_forest_paths(f, tree_of, indices, count, paths);
}
int zl_merkle_forest_tree_nodes(const zl_merkle_forest* f, uint32_t tree, const void** nodes) {
    if (!f || !nodes || tree >= f->trees) return ZL_EINVAL;
    *nodes = f->nodes + (size_t)tree * f->stride * 4;
    return ZL_OK;
}
int zl_merkle_forest_download(const zl_merkle_forest* f, uint32_t tree, uint64_t* nodes) {
    if (!f || !nodes || tree >= f->trees) return ZL_EINVAL;
    const uint64_t* from = f->nodes + (size_t)tree * f->stride * 4;
    if (!f->ctx) {
        memcpy(nodes, from, f->stride * 32);
        return ZL_OK;
    }
    zl_ctx* ctx = f->ctx;
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    ZL_HIP(ctx, hipMemcpyAsync(nodes, from, f->stride * 32, hipMemcpyDeviceToHost, ctx->stream));
    ZL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZL_OK;
}
int zl_merkle_forest_member_assignments_dev(const zl_merkle_forest* f, const uint32_t* tree_of, const uint64_t* indices, size_t count, void* d_out, size_t stride_elems) {
    if (!f || !f->ctx || stride_elems < pd::merkle_row_elems(f->depth) || (count && (!tree_of || !indices || !d_out)) || ((uintptr_t)d_out & 15) ||
        forest_members_ok(f, tree_of, indices, count))
        return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    ZL_HIP(f->ctx, hipSetDevice(f->ctx->device));
    return ZL_POS_CURVE(f->curve, dev_merkle_from_forest, f->ctx, f, tree_of, indices, count, d_out, stride_elems, nullptr, nullptr);
}

}  // extern "C"

int zl_merkle_forest_prover_view(const zl_merkle_forest* f, const zl_ctx* ctx, int* curve, unsigned* depth) {
    if (!f || !f->ctx || !ctx || ctx->device != f->ctx->device) return ZL_EINVAL;
    *curve = (int)f->curve;
    *depth = f->depth;
    return ZL_OK;
}
int zl_merkle_forest_members_ok(const zl_merkle_forest* f, const uint32_t* tree_of, const uint64_t* indices, size_t count) {
    return forest_members_ok(f, tree_of, indices, count);
}
int zl_merkle_forest_member_rows(zl_ctx* ctx, const zl_merkle_forest* f, const uint32_t* tree_of, const uint64_t* indices, size_t count, void* d_rows, size_t stride_elems,
                                 uint64_t* host_rows, uint64_t* roots_out) {
    return ZL_POS_CURVE(f->curve, dev_merkle_from_forest, ctx, f, tree_of, indices, count, d_rows, stride_elems, host_rows, roots_out);
}
