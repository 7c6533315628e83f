// zl_edwards_dev.hip -- scalar multiplication on the two embedded twisted Edwards curves (zl_edwards.h) and the hybrid Diffie-Hellman / Poseidon-duplex encryption
// on top of it (include/zl_backend_ext.h): the reference's encryption::hybrid::Hybrid<DiffieHellman, FixedDuplexer>.  One unit for both curves,
// built with the multiplier inlined (ZL_INLINE_MUL_DEVICE); a host mirror -- the SAME templates of zl_edwards.h over the library's thread pool -- behind the same
// entry points, so results are byte-identical on every path.
//
// Kernels (templates over the scalar-field parameters FrP of the pairing curve, which is the embedded curve's base field), one lane per item, 64 lanes a block:
//   k_ed_mul<FrP, UK>   k P for the lane's own point: range and on-curve test (4 products), the 16-entry table 0 P .. 15 P of the lane in the unit's scratch slot
//                    (ZL_SLOT_EDWARDS; laid out entry-major, then limb-major, across the 64 lanes of the block: word (e, c, k) of lane t at ((e * 4 + c) * 9 + k) * 64 + t,
//                    so a wave's table writes are 256-byte rows and a digit is an index, never a branch), 63 four-bit windows of 4 doublings and one unified
//                    addition, with ZL_ED_CHECK_SUBGROUP the same loop once more for l P, one Fermat inversion, canonical store.  UK: every lane has the SAME scalar
//                    (scalar_stride == 0, the scan with one viewing key): its address is the kernel argument, so the digits -- the scalar's own nibbles, unsigned
//                    windows need no recoding -- come through wave-uniform loads.
//   k_ed_mul_fixed<FrP>  k P for ONE point shared by the call (point_stride == 0): the host mirror builds the 63 x 16 table d 16^w P once per call, affine with d x y
//                    precomputed (batch-inverted: one inversion), uploads it once, and every lane does 63 mixed additions and no doubling.
//   k_ed_mul_trace<FrP>  the complete assignment of zl_circuit_ed_scalar_mul per item (ed::trace_item): the double-and-add ladder of the in-circuit gadget in extended
//                    coordinates, ONE inversion a lane, every affine record by Montgomery's trick; no table, no scratch slot.
//   k_ed_hybrid_ladders<FrP>  the embedded-curve part of zl_circuit_hybrid_encrypt's assignment: ONE LANE PER (row, ladder) -- blockIdx.y says which, so it is wave-uniform:
//                    the ladder over G (and the row's head: 1, G, pk, esk, the bits, epk) or the ladder over pk, whose result cells are the cipher's key.  Both run
//                    ed::ladder_cells, k_ed_mul_trace's body; the cipher's cells are k_pos_duplex_trace_in's, launched behind it on the same stream.
// A lane at or above the item count returns before it reads or writes anything; a table is only touched by the lane that owns it.
#include <string.h>
#include <atomic>
#include <functional>
#include <vector>
#include "zl_ctx.h"
#include "zl_edwards.h"
#include "zl_edwards_dev.h"
#include "zl_poseidon_dev.h"

using namespace openzl;

namespace {
constexpr int BLOCK = 64;
// knob defaults: ZL_TUNE_ED_CHUNK / _DEV_MIN / _FIXED_MIN (README).  DEV_MIN and FIXED_MIN rest on MEASUREMENTS (profiles/edwards_bench.log): each
// is the smallest power of two from which the new path won every repetition on both curves -- the device against the host pool (a launch is the 1.46 ms of ONE
// multiplication whatever its width; the pool still wins at 128 items, x 0.89 - 0.97), the fixed-base kernel against k_ed_mul from the smallest size measured.
constexpr int DEFAULT_CHUNK = 1 << 16, DEFAULT_DEV_MIN = 256, DEFAULT_FIXED_MIN = 64;
constexpr size_t STAGE_BUDGET = (size_t)256 << 20;  // bytes of ZL_SLOT_EDWARDS one chunk may take: tables (2304 B a lane) and staged operands
constexpr size_t FLAG_BYTES = 256;
constexpr int FIXED_ENTRY_WORDS = 3 * ed::LIMBS;    // x, y, d x y
constexpr size_t FIXED_TABLE_BYTES = (size_t)ed::WINDOWS * ed::TABLE * FIXED_ENTRY_WORDS * 4;  // 108 864 B

bool valid_curve(zl_curve_t c) { return c == ZL_BLS12_381 || c == ZL_BN254; }
constexpr size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
unsigned blocks_of(size_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

// ---------------------------------------------------------------------------------------------------------------- device
// the lane's table in the block's region: `base` already points at the lane's column
template <class FrP>
struct DevTab {
    uint32_t* base;
    __device__ __forceinline__ void put(int e, const ed::Pt<FrP>& p) {
        uint32_t* w = base + (size_t)e * ed::POINT_WORDS * BLOCK;
#pragma unroll
        for (int k = 0; k < ed::LIMBS; k++) {
            w[(0 * ed::LIMBS + k) * BLOCK] = p.X.l[k];
            w[(1 * ed::LIMBS + k) * BLOCK] = p.Y.l[k];
            w[(2 * ed::LIMBS + k) * BLOCK] = p.Z.l[k];
            w[(3 * ed::LIMBS + k) * BLOCK] = p.T.l[k];
        }
    }
    __device__ __forceinline__ ed::Pt<FrP> get(int e) const {
        const uint32_t* w = base + (size_t)e * ed::POINT_WORDS * BLOCK;
        ed::Pt<FrP> p;
#pragma unroll
        for (int k = 0; k < ed::LIMBS; k++) {
            p.X.l[k] = w[(0 * ed::LIMBS + k) * BLOCK];
            p.Y.l[k] = w[(1 * ed::LIMBS + k) * BLOCK];
            p.Z.l[k] = w[(2 * ed::LIMBS + k) * BLOCK];
            p.T.l[k] = w[(3 * ed::LIMBS + k) * BLOCK];
        }
        return p;
    }
};
static_assert(ed::LIMBS == ed::El<BLS12_381_Fr>::L && ed::LIMBS == ed::El<BN254_Fr>::L, "nine limbs an element");
// what a lane leaves behind: the point, and its status -- kept when an earlier launch of the call already refused the item (`keep`), raised through the flag
// word when the caller asked for no status array
__device__ __forceinline__ void finish_item(size_t p, uint8_t st, const uint64_t* o, uint64_t* __restrict__ out, uint8_t* __restrict__ status, bool keep,
                                            uint32_t* __restrict__ flag) {
    const bool refused = keep && status && status[p] != 0;
    if (refused) st = status[p];
#pragma unroll
    for (int i = 0; i < 8; i++) out[p * 8 + i] = refused ? (i == 4 ? 1 : 0) : o[i];
    if (status) status[p] = st;
    else if (st) atomicOr(flag, 1u);
}
// tables: blocks x 16 x 36 x 64 words, block b's region at b * 16 * 36 * 64
template <class FrP, bool UK>
__global__ __launch_bounds__(BLOCK) void k_ed_mul(const uint64_t* __restrict__ points, uint32_t point_stride, const uint64_t* __restrict__ scalars, size_t n, bool check_subgroup,
                                                  uint32_t* __restrict__ tables, uint64_t* __restrict__ out, uint8_t* __restrict__ status, bool keep, uint32_t* __restrict__ flag) {
    const size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    DevTab<FrP> tab{tables + (size_t)blockIdx.x * (ed::TABLE * ed::POINT_WORDS * BLOCK) + threadIdx.x};
    uint64_t o[8];
    const uint8_t st = ed::mul_item<FrP>(points + p * point_stride * 8, UK ? scalars : scalars + p * 4, check_subgroup, tab, o);
    finish_item(p, st, o, out, status, keep, flag);
}
// table: 63 x 16 entries of 27 words (x, y, d x y as limbs of x R'), entry (w, e) = e 16^w P; point_status: what the host found of P (range, curve, subgroup)
template <class FrP>
__global__ __launch_bounds__(BLOCK) void k_ed_mul_fixed(const uint32_t* __restrict__ table, const uint64_t* __restrict__ scalars, uint32_t scalar_stride, size_t n,
                                                        uint32_t point_status, uint64_t* __restrict__ out, uint8_t* __restrict__ status, bool keep, uint32_t* __restrict__ flag) {
    const size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint64_t* k = scalars + p * scalar_stride * 4;
    ed::Pt<FrP> acc = ed::identity<FrP>();
#pragma unroll 1
    for (int w = 0; w < ed::WINDOWS; w++) {
        const uint32_t* e = table + ((size_t)w * ed::TABLE + ed::digit_of(k, w)) * FIXED_ENTRY_WORDS;
        ed::El<FrP> x, y, dt;
#pragma unroll
        for (int i = 0; i < ed::LIMBS; i++) {
            x.l[i] = e[i];
            y.l[i] = e[ed::LIMBS + i];
            dt.l[i] = e[2 * ed::LIMBS + i];
        }
        acc = ed::madd<FrP>(acc, x, y, dt);
    }
    uint64_t o[8];
    const uint8_t st = point_status ? (uint8_t)point_status : ed::scalar_ok<FrP>(k) ? ed::ST_OK : ed::ST_SCALAR;
    if (st == ed::ST_OK) ed::store_affine<FrP>(o, acc);
    else ed::store_identity(o);
    finish_item(p, st, o, out, status, keep, flag);
}

// The complete assignment of zl_circuit_ed_scalar_mul per item, one lane a row (ed::trace_item: the ladder in extended coordinates, ONE inversion a lane, the
// affine records by Montgomery's trick -- the points kept between the passes live in the row's own not yet written step cells, so the kernel needs no scratch
// slot).  Row p = out + p * stride elements, 16-byte aligned; a lane stores its 32-byte records directly at a stride of one row, the layout k_pos_chain_trace
// kept (profiles/chain_trace_layout_ab.log: staging a block's records through LDS lost 12 - 15 % up to 2^16 rows); elements behind the row are not touched.
// q_out (may be null): Q of every item, densely.  Rows and inputs do not overlap.
template <class FrP>
__global__ __launch_bounds__(BLOCK) void k_ed_mul_trace(const uint64_t* __restrict__ points, uint32_t point_stride, const uint64_t* __restrict__ scalars, uint32_t bits, size_t n,
                                                        uint64_t* __restrict__ out, size_t stride, uint64_t* __restrict__ q_out, uint32_t* __restrict__ flag) {
    const size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const bool ok = ed::trace_item<FrP>(points + p * point_stride * 8, scalars + p * 4, bits, out + p * stride * 4, q_out ? q_out + p * 8 : nullptr);
    if (!ok) atomicOr(flag, 1u);
}

// The two ladders of zl_circuit_hybrid_encrypt's rows (ed::hybrid_ladder_item), one lane per (row, ladder): the grid is blocks_of(n) x 2 and blockIdx.y is the
// ladder, so a wave runs one ladder only and the shared G comes through uniform loads (the branch below is on a wave-uniform value; the body is ONE copy).  A
// lane that ran both ladders in series would pay the launch's latency twice: the two depend only on esk's bits.  The G lane (y = 0) also writes the row's head and
// epk (and epk_out, may be null, densely); the pk lane (y = 1) writes its ladder's cells and nothing else.  Row p = out + p * stride elements, 16-byte aligned;
// cells behind the pk ladder are the cipher launch's.  No scratch slot, as k_ed_mul_trace.
template <class FrP>
__global__ __launch_bounds__(BLOCK) void k_ed_hybrid_ladders(const uint64_t* __restrict__ g, const uint64_t* __restrict__ pks, uint32_t pk_stride, const uint64_t* __restrict__ esk,
                                                             const ed::HybridRow lay, size_t n, uint64_t* __restrict__ out, size_t stride, uint64_t* __restrict__ epk_out,
                                                             uint32_t* __restrict__ flag) {
    const size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const int which = (int)blockIdx.y;
    const uint64_t* pk = pks + p * pk_stride * 8;
    uint64_t w[8];
    if (which == 0) {
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = g[i];
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = pk[i];
    }
    const bool ok = ed::hybrid_ladder_item<FrP>(w, pk, esk + p * 4, lay, which, out + p * stride * 4, epk_out ? epk_out + p * 8 : nullptr);
    if (!ok) atomicOr(flag, 1u);
}

// ---------------------------------------------------------------------------------------------------------------- host mirror
template <class Fn>
void host_for(size_t n, const Fn& f) {
    constexpr size_t B = 8;
    const std::function<void(size_t)> g = [&](size_t b) {
        const size_t end = (b + 1) * B < n ? (b + 1) * B : n;
        for (size_t i = b * B; i < end; i++) f(i);
    };
    zl_pool_get().parallel_for((n + B - 1) / B, g);
}
template <class FrP>
uint8_t host_item(const uint64_t* p_xy, const uint64_t* k, bool check, uint64_t* out_xy) {
    ed::LocalTab<FrP> tab;
    return ed::mul_item<FrP>(p_xy, k, check, tab, out_xy);
}
// status may be null: then the return value says whether every item was accepted
template <class FrP>
int host_mul(const uint64_t* points, size_t ps, const uint64_t* scalars, size_t ks, size_t count, bool check, uint64_t* out, uint8_t* status, bool keep) {
    std::atomic<int> bad{0};
    host_for(count, [&](size_t i) {
        uint64_t o[8];
        uint8_t st = host_item<FrP>(points + i * ps * 8, scalars + i * ks * 4, check, o);
        if (keep && status && status[i]) {
            st = status[i];
            ed::store_identity(o);
        }
        memcpy(out + i * 8, o, 64);
        if (status) status[i] = st;
        else if (st) bad.store(1);
    });
    return bad.load() ? ZL_EINVAL : ZL_OK;
}
template <class FrP>
int host_add(const uint64_t* p, const uint64_t* q, uint64_t* out) {
    ed::El<FrP> px, py, qx, qy;
    bool ok = ed::load<FrP>(p, px);
    ok &= ed::load<FrP>(p + 4, py);
    ok &= ed::load<FrP>(q, qx);
    ok &= ed::load<FrP>(q + 4, qy);
    if (!ok || !ed::on_curve<FrP>(px, py) || !ed::on_curve<FrP>(qx, qy)) return ZL_EINVAL;
    ed::store_affine<FrP>(out, ed::add<FrP>(ed::from_affine<FrP>(px, py), ed::from_affine<FrP>(qx, qy), ed::coeff_d<FrP>()));
    return ZL_OK;
}
template <class FrP>
int params_out(uint64_t* a, uint64_t* d, uint64_t* order, uint64_t* cofactor) {
    if (a) {
        if (ed::Curve<FrP>::A > 0) {
            a[0] = 1;
            a[1] = a[2] = a[3] = 0;
        } else {
            for (int i = 0; i < 4; i++) a[i] = (uint64_t)FrP::mod(2 * i) | ((uint64_t)FrP::mod(2 * i + 1) << 32);
            a[0] -= 1;  // (q is odd: no borrow)
        }
    }
    for (int i = 0; i < 4; i++) {
        if (d) d[i] = (uint64_t)ed::Curve<FrP>::d(2 * i) | ((uint64_t)ed::Curve<FrP>::d(2 * i + 1) << 32);
        if (order) order[i] = (uint64_t)ed::Curve<FrP>::l(2 * i) | ((uint64_t)ed::Curve<FrP>::l(2 * i + 1) << 32);
        if (cofactor) cofactor[i] = i ? 0 : ed::COFACTOR;
    }
    return ZL_OK;
}
// The fixed-base table of P, and what is wrong with P (0: nothing).  Row w holds e 16^w P, e = 0 .. 15: row 0 by repeated addition, the base of row w + 1 by
// four doublings of row w's; all 1008 points are then made affine with ONE inversion (Montgomery's trick) and stored as the limbs of x, y and d x y.
template <class FrP>
uint8_t host_fixed_table(const uint64_t* p_xy, bool check, std::vector<uint32_t>& words) {
    constexpr int N = ed::WINDOWS * ed::TABLE;
    words.assign((size_t)N * FIXED_ENTRY_WORDS, 0u);
    ed::El<FrP> x, y;
    bool in_range = ed::load<FrP>(p_xy, x);
    in_range &= ed::load<FrP>(p_xy + 4, y);
    if (!in_range) return ed::ST_RANGE;
    if (!ed::on_curve<FrP>(x, y)) return ed::ST_CURVE;
    const ed::El<FrP> d = ed::coeff_d<FrP>();
    if (check) {
        ed::LocalTab<FrP> tab;
        ed::build_table<FrP>(tab, ed::from_affine<FrP>(x, y), d);
        if (!ed::is_identity<FrP>(ed::window_mul<FrP>(tab, nullptr, d))) return ed::ST_SUBGROUP;
    }
    std::vector<ed::Pt<FrP>> pts((size_t)N);
    ed::Pt<FrP> base = ed::from_affine<FrP>(x, y);
    for (int w = 0; w < ed::WINDOWS; w++) {
        ed::Pt<FrP>* row = pts.data() + (size_t)w * ed::TABLE;
        row[0] = ed::identity<FrP>();
        row[1] = base;
        for (int e = 2; e < ed::TABLE; e++) row[e] = ed::add<FrP>(row[e - 1], base, d);
        for (int j = 0; j < ed::WINDOW; j++) base = ed::dbl<FrP>(base, j == ed::WINDOW - 1);
    }
    std::vector<ed::El<FrP>> pre((size_t)N);  // pre[i] = Z_0 .. Z_i
    pre[0] = pts[0].Z;
    for (int i = 1; i < N; i++) pre[(size_t)i] = zl::mul(pre[(size_t)i - 1], pts[(size_t)i].Z);
    ed::El<FrP> run = ed::inv<FrP>(pre[(size_t)N - 1]);  // (no Z is zero: the law is complete)
    for (int i = N - 1; i >= 0; i--) {
        const ed::El<FrP> zi = i ? zl::mul(run, pre[(size_t)i - 1]) : run;
        run = zl::mul(run, pts[(size_t)i].Z);
        // canonical limbs of the affine coordinates back in the multiplier's form: what a LOADED affine point is, so the mixed addition's bounds are add's
        uint64_t c[8];
        ed::store<FrP>(c, zl::mul(pts[(size_t)i].X, zi));
        ed::store<FrP>(c + 4, zl::mul(pts[(size_t)i].Y, zi));
        ed::El<FrP> ax, ay;
        (void)ed::load<FrP>(c, ax);
        (void)ed::load<FrP>(c + 4, ay);
        const ed::El<FrP> dt = zl::mul(d, zl::mul(ax, ay));
        uint32_t* o = words.data() + (size_t)i * FIXED_ENTRY_WORDS;
        for (int k = 0; k < ed::LIMBS; k++) {
            o[k] = ax.l[k];
            o[ed::LIMBS + k] = ay.l[k];
            o[2 * ed::LIMBS + k] = dt.l[k];
        }
    }
    return ed::ST_OK;
}

// ---------------------------------------------------------------------------------------------------------------- device path: chunks over the unit's slot
size_t tune_chunk() {
    const int c = zl_tune("ZL_TUNE_ED_CHUNK", DEFAULT_CHUNK);
    const size_t v = c < BLOCK ? (size_t)BLOCK : c > (1 << 20) ? (size_t)1 << 20 : (size_t)c;
    return v / BLOCK * BLOCK;  // whole blocks: a block's table region belongs to one launch
}
bool on_host(const zl_ctx* ctx, size_t count) {
    if (!ctx) return true;
    const int m = zl_tune("ZL_TUNE_ED_DEV_MIN", DEFAULT_DEV_MIN);
    return m > 0 && count < (size_t)m;
}
bool use_fixed(size_t point_stride, size_t count) {
    const int m = zl_tune("ZL_TUNE_ED_FIXED_MIN", DEFAULT_FIXED_MIN);
    return point_stride == 0 && m >= 0 && count >= (size_t)(m > 0 ? m : 1);
}
#define ZL_ED_LAUNCH(ctx, kernel, grid, ...)                                              \
    do {                                                                                  \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(BLOCK), 0, (ctx)->stream, __VA_ARGS__); \
        ZL_HIP(ctx, hipGetLastError());                                                   \
    } while (0)

// One operand of a chunked call.  Staged (host == true): `per` bytes per item in the slot -- or, per == 0, `once` bytes for the whole call, uploaded in front of
// the first chunk -- uploaded from `up` and downloaded to `down` (host memory, either may be null: a scratch-only operand).  Otherwise `dev` is the caller's
// device memory and a chunk starting at item `first` finds its part at dev + first * per.  per == 0 and once == 0: absent, a null pointer.
struct Seg {
    bool host;
    size_t per, once;
    const void* up;
    void* down;
    void* dev;
};
Seg staged(size_t per, const void* up, void* down) { return Seg{true, per, 0, up, down, nullptr}; }
Seg staged_once(size_t bytes, const void* up) { return Seg{true, 0, bytes, up, nullptr, nullptr}; }
Seg device(size_t per, const void* dev) { return Seg{false, per, 0, nullptr, nullptr, const_cast<void*>(dev)}; }
constexpr size_t MAX_SEGS = 12;
// Runs `count` items in chunks on ctx's stream: a chunk is at most ZL_TUNE_ED_CHUNK lanes, cut so that its tables and staged operands fit STAGE_BUDGET.  Per
// chunk, in stream order: the uploads, launch(first, m, d, tables, flag), the downloads.  The flag word is cleared once and read once, at the end; finished on
// return -- also when a HIP call or `launch` fails: run_chunks drains the stream before it hands the error on, so no queued copy still targets the caller's
// (or a caller's local) host memory.
template <class Launch>
int run_chunks_issue(zl_ctx* ctx, size_t count, bool tables, const std::vector<Seg>& segs, const Launch& launch) {
    if (segs.size() > MAX_SEGS) return ZL_EINVAL;
    size_t per = tables ? ed::TABLE_BYTES : 0, once = 0;
    for (const Seg& g : segs)
        if (g.host) {
            per += g.per;
            once += up256(g.once);
        }
    size_t chunk = tune_chunk();
    if (per) {
        const size_t by_budget = (STAGE_BUDGET - (once < STAGE_BUDGET / 2 ? once : STAGE_BUDGET / 2)) / per / BLOCK * BLOCK;
        if (by_budget < chunk) chunk = by_budget ? by_budget : BLOCK;
    }
    const size_t m0 = count < chunk ? count : chunk, lanes0 = (size_t)blocks_of(m0) * BLOCK;
    size_t off[MAX_SEGS + 1] = {0};
    size_t total = FLAG_BYTES + (tables ? up256(lanes0 * ed::TABLE_BYTES) : 0);
    for (size_t j = 0; j < segs.size(); j++) {
        off[j] = total;
        if (segs[j].host) total += up256(segs[j].per ? m0 * segs[j].per : segs[j].once);
    }
    void* slot = nullptr;
    int rc = zl_scratch_get(ctx, ZL_SLOT_EDWARDS, total, &slot);
    if (rc) return rc;
    unsigned char* base = static_cast<unsigned char*>(slot);
    uint32_t* flag = static_cast<uint32_t*>(slot);
    uint32_t* d_tables = tables ? reinterpret_cast<uint32_t*>(base + FLAG_BYTES) : nullptr;
    ZL_HIP(ctx, hipMemsetAsync(flag, 0, 4, ctx->stream));
    for (size_t j = 0; j < segs.size(); j++)
        if (segs[j].host && !segs[j].per && segs[j].once && segs[j].up) ZL_HIP(ctx, hipMemcpyAsync(base + off[j], segs[j].up, segs[j].once, hipMemcpyHostToDevice, ctx->stream));
    for (size_t first = 0; first < count; first += chunk) {
        const size_t m = count - first < chunk ? count - first : chunk;
        void* d[MAX_SEGS] = {};
        for (size_t j = 0; j < segs.size(); j++) {
            const Seg& g = segs[j];
            if (g.host) {
                d[j] = g.per || g.once ? base + off[j] : nullptr;
                if (g.per && g.up)
                    ZL_HIP(ctx, hipMemcpyAsync(d[j], static_cast<const unsigned char*>(g.up) + first * g.per, m * g.per, hipMemcpyHostToDevice, ctx->stream));
            } else {
                d[j] = g.dev ? static_cast<unsigned char*>(g.dev) + first * g.per : nullptr;
            }
        }
        if ((rc = launch(first, m, d, d_tables, flag))) return rc;
        for (size_t j = 0; j < segs.size(); j++)
            if (segs[j].host && segs[j].per && segs[j].down)
                ZL_HIP(ctx, hipMemcpyAsync(static_cast<unsigned char*>(segs[j].down) + first * segs[j].per, d[j], m * segs[j].per, hipMemcpyDeviceToHost, ctx->stream));
    }
    uint32_t bad = 0;
    ZL_HIP(ctx, hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    ZL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return bad ? ZL_EINVAL : ZL_OK;
}
template <class Launch>
int run_chunks(zl_ctx* ctx, size_t count, bool tables, const std::vector<Seg>& segs, const Launch& launch) {
    const int rc = run_chunks_issue(ctx, count, tables, segs, launch);
    if (rc) (void)hipStreamSynchronize(ctx->stream);  // (ZL_EINVAL from the flag word has synchronised already: a second wait returns at once)
    return rc;
}
uint64_t* u64(void* p) { return static_cast<uint64_t*>(p); }
uint8_t* u8(void* p) { return static_cast<uint8_t*>(p); }

// one multiplication launch over m items: the fixed-base kernel when the call built a table, else k_ed_mul
struct MulCall {
    bool check;
    size_t ps, ks;
    const uint32_t* d_fixed;  // the uploaded fixed-base table, or null
    uint8_t point_status;      // ... and what the host found of its point
};
template <class FrP>
int launch_mul(zl_ctx* ctx, const MulCall& c, const uint64_t* d_points, const uint64_t* d_scalars, size_t m, uint32_t* d_tables, uint64_t* d_out, uint8_t* d_status, bool keep,
               uint32_t* flag) {
    if (c.d_fixed)
        ZL_ED_LAUNCH(ctx, (k_ed_mul_fixed<FrP>), blocks_of(m), c.d_fixed, d_scalars, (uint32_t)c.ks, m, (uint32_t)c.point_status, d_out, d_status, keep, flag);
    else if (c.ks == 0)
        ZL_ED_LAUNCH(ctx, (k_ed_mul<FrP, true>), blocks_of(m), d_points, (uint32_t)c.ps, d_scalars, m, c.check, d_tables, d_out, d_status, keep, flag);
    else
        ZL_ED_LAUNCH(ctx, (k_ed_mul<FrP, false>), blocks_of(m), d_points, (uint32_t)c.ps, d_scalars, m, c.check, d_tables, d_out, d_status, keep, flag);
    return ZL_OK;
}
// zl_ed_scalar_mul_batch on the device.  on_host_ptrs: points, scalars, out and status are host memory and staged; else the caller's device memory.
template <class FrP>
int dev_mul(zl_ctx* ctx, bool on_host_ptrs, const uint64_t* points, size_t ps, const uint64_t* scalars, size_t ks, size_t count, bool check, uint64_t* out, uint8_t* status) {
    std::vector<uint32_t> fixed;
    uint8_t pst = 0;
    const bool fx = use_fixed(ps, count);
    if (fx) {
        uint64_t pxy[8];
        if (on_host_ptrs) memcpy(pxy, points, 64);
        else {  // the table is built on the host: the point comes down on the ctx's stream, behind whatever the caller queued there
            ZL_HIP(ctx, hipMemcpyAsync(pxy, points, 64, hipMemcpyDeviceToHost, ctx->stream));
            ZL_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        pst = host_fixed_table<FrP>(pxy, check, fixed);
    }
    std::vector<Seg> segs;
    if (on_host_ptrs) {
        segs = {ps ? staged(64, points, nullptr) : staged_once(64, points), ks ? staged(32, scalars, nullptr) : staged_once(32, scalars), staged(64, nullptr, out),
                staged(status ? 1 : 0, nullptr, status)};
    } else {
        segs = {device(ps * 64, points), device(ks * 32, scalars), device(64, out), device(1, status)};
    }
    segs.push_back(staged_once(fx ? FIXED_TABLE_BYTES : 0, fixed.data()));
    return run_chunks(ctx, count, !fx, segs, [&](size_t, size_t m, void* const* d, uint32_t* tables, uint32_t* flag) -> int {
        const MulCall c{check, ps, ks, fx ? static_cast<const uint32_t*>(d[4]) : nullptr, pst};
        return launch_mul<FrP>(ctx, c, u64(d[0]), u64(d[1]), m, tables, u64(d[2]), u8(d[3]), false, flag);
    });
}

// ---- the scalar-multiplication circuit's assignments: the kernel's text over the host pool, or the kernel
template <class FrP>
int host_trace(const uint64_t* points, size_t ps, const uint64_t* scalars, unsigned bits, size_t count, uint64_t* out, size_t nv) {
    std::atomic<int> bad{0};
    host_for(count, [&](size_t i) {
        if (!ed::trace_item<FrP>(points + i * ps * 8, scalars + i * 4, bits, out + i * nv * 4, nullptr)) bad.store(1);
    });
    return bad.load() ? ZL_EINVAL : ZL_OK;
}
// Every device form.  points / scalars: staged per chunk when in_on_host, else device memory; host_rows != null: the rows are staged, dense, and downloaded
// (d_rows and stride are ignored), otherwise row i goes to d_rows + i * stride elements; host_q != null: Q of every item is staged and downloaded.  A chunk is
// one launch; a staged row counts nv * 32 bytes against the budget, so a full-width call of host rows runs about 2 300 rows a chunk.
template <class FrP>
int trace_run(zl_ctx* ctx, const uint64_t* points, size_t ps, const uint64_t* scalars, bool in_on_host, unsigned bits, size_t count, uint64_t* d_rows, size_t stride,
              uint64_t* host_rows, uint64_t* host_q) {
    const size_t nv = ed::trace_row_elems(bits);
    std::vector<Seg> segs;
    if (in_on_host) segs = {ps ? staged(64, points, nullptr) : staged_once(64, points), staged(32, scalars, nullptr)};
    else segs = {device(ps * 64, points), device(32, scalars)};
    segs.push_back(host_rows ? staged(nv * 32, nullptr, host_rows) : device(stride * 32, d_rows));
    segs.push_back(staged(host_q ? 64 : 0, nullptr, host_q));
    return run_chunks(ctx, count, false, segs, [&](size_t, size_t m, void* const* d, uint32_t*, uint32_t* flag) -> int {
        ZL_ED_LAUNCH(ctx, (k_ed_mul_trace<FrP>), blocks_of(m), u64(d[0]), (uint32_t)ps, u64(d[1]), (uint32_t)bits, m, u64(d[2]), host_rows ? nv : stride, u64(d[3]), flag);
        return ZL_OK;
    });
}
template <class FrP>
size_t trace_elems(unsigned bits) {
    return bits >= 1 && bits <= ed::order_bits<FrP>() ? ed::trace_row_elems(bits) : 0;
}

// ---- the hybrid-encryption circuit's assignments.  What a call is, beside its operands: checked by hybrid_trace_params, init the W canonical elements
struct HybridTrace {
    zl_curve_t curve;
    unsigned width;
    uint64_t init[4 * poseidon_dev::MAX_WIDTH];
    size_t H, N;
    ed::HybridRow row;
    zl_duplex_row_layout cipher() const { return zl_duplex_row_layout{7, 8, 8 + row.T, row.key_at(), row.plain_at(), row.rec_at()}; }
};
// 0 elements for a parameter out of range: the curve, the cipher's limits at key_len = 2, 1 <= bits <= the order's length
size_t hybrid_trace_elems(zl_curve_t curve, unsigned width, unsigned bits, size_t H, size_t N, ed::HybridRow* row_out) {
    namespace pd = poseidon_dev;
    if (!valid_curve(curve) || !pd::encrypt_shape_ok(width, 2, H, N) || bits < 1 || bits > (curve == ZL_BLS12_381 ? ed::order_bits<BLS12_381_Fr>() : ed::order_bits<BN254_Fr>()))
        return 0;
    const ed::HybridRow row{bits, N * (width - 1), H, pd::encrypt_sboxes(width, 2, H, N)};
    if (row_out) *row_out = row;
    return row.elems();
}
static_assert(27 * 252 - 13 + 2 * 1024 * 5 + 64 + 3 * poseidon_dev::encrypt_sboxes(6, 2, 64, 1024) < ((size_t)1 << 31), "the longest row fits 31 bits");
template <class FrP>
bool generator_ok(const uint64_t* g) {
    ed::El<FrP> x, y;
    bool ok = ed::load<FrP>(g, x);
    ok &= ed::load<FrP>(g + 4, y);
    return ok && ed::on_curve<FrP>(x, y);
}
// the parameters, the initial state and G, on the host before any work
int hybrid_trace_params(zl_curve_t curve, unsigned width, unsigned bits, const uint64_t* initial_state, const uint64_t* g, size_t H, size_t N, HybridTrace* c) {
    c->curve = curve;
    c->width = width;
    c->H = H;
    c->N = N;
    if (hybrid_trace_elems(curve, width, bits, H, N, &c->row) == 0 || !g) return ZL_EINVAL;
    if (zl_poseidon_duplex_row_params((int)curve, width, initial_state, 2, H, N, c->init)) return ZL_EINVAL;
    return (curve == ZL_BLS12_381 ? generator_ok<BLS12_381_Fr>(g) : generator_ok<BN254_Fr>(g)) ? ZL_OK : ZL_EINVAL;
}
// host mirror: the 2 count ladders over the pool (the kernel's text), then the cipher's host rows with the key read from each row's S cells
template <class FrP>
int host_hybrid_trace(const HybridTrace& c, const uint64_t* g, const uint64_t* esk, const uint64_t* pks, size_t ps, const uint64_t* headers, const uint64_t* texts, size_t count,
                      uint64_t* out) {
    const size_t nv = c.row.elems();
    std::atomic<int> bad{0};
    host_for(2 * count, [&](size_t j) {
        const size_t i = j >> 1;
        const int which = (int)(j & 1);
        const uint64_t* pk = pks + i * ps * 8;
        if (!ed::hybrid_ladder_item<FrP>(which ? pk : g, pk, esk + i * 4, c.row, which, out + i * nv * 4, nullptr)) bad.store(1);
    });
    const int rc = zl_poseidon_duplex_row_host((int)c.curve, c.width, c.init, c.cipher(), 2, headers, c.H, texts, c.N, count, out, nv);
    return rc ? rc : bad.load() ? ZL_EINVAL : ZL_OK;
}
// Every device form.  esk / pks / headers / texts: staged per chunk when in_on_host, else device memory; g: host memory in every form, uploaded once;
// host_rows != null: the rows are staged, dense, and downloaded (d_rows and stride are ignored), otherwise row i goes to d_rows + i * stride elements; host_epk /
// host_tags / host_cts != null: epk, tag and ciphertext of every item are staged and downloaded.  A chunk is two launches on the ctx's stream: the ladders
// (2 m lanes), then the cipher over the same rows -- through ZL_SLOT_EDWARDS alone: the cipher launch stages nothing.
template <class FrP>
int hybrid_trace_run(zl_ctx* ctx, const HybridTrace& c, const uint64_t* g, const uint64_t* esk, const uint64_t* pks, size_t ps, const uint64_t* headers, const uint64_t* texts,
                     bool in_on_host, size_t count, uint64_t* d_rows, size_t stride, uint64_t* host_rows, uint64_t* host_epk, uint64_t* host_tags, uint64_t* host_cts) {
    const size_t nv = c.row.elems(), T = c.row.T;
    std::vector<Seg> segs;
    if (in_on_host) segs = {staged(32, esk, nullptr), ps ? staged(64, pks, nullptr) : staged_once(64, pks), staged(c.H * 32, headers, nullptr), staged(T * 32, texts, nullptr)};
    else segs = {device(32, esk), device(ps * 64, pks), device(c.H * 32, headers), device(T * 32, texts)};
    segs.push_back(staged_once(64, g));                                                                      // 4
    segs.push_back(host_rows ? staged(nv * 32, nullptr, host_rows) : device(stride * 32, d_rows));           // 5
    segs.push_back(staged(host_epk ? 64 : 0, nullptr, host_epk));                                            // 6
    segs.push_back(staged(host_tags ? 32 : 0, nullptr, host_tags));                                          // 7
    segs.push_back(staged(host_cts ? T * 32 : 0, nullptr, host_cts));                                        // 8
    const zl_duplex_row_layout lay = c.cipher();
    return run_chunks(ctx, count, false, segs, [&](size_t, size_t m, void* const* d, uint32_t*, uint32_t* flag) -> int {
        const size_t st = host_rows ? nv : stride;
        hipLaunchKernelGGL((k_ed_hybrid_ladders<FrP>), dim3(blocks_of(m), 2), dim3(BLOCK), 0, ctx->stream, u64(d[4]), u64(d[1]), (uint32_t)ps, u64(d[0]), c.row, m, u64(d[5]), st,
                           u64(d[6]), flag);
        ZL_HIP(ctx, hipGetLastError());
        return zl_poseidon_duplex_row_launch(ctx, (int)c.curve, c.width, c.init, lay, 2, d[2], c.H, d[3], c.N, m, d[5], st, d[7], d[8], flag);
    });
}

// ---- hybrid encryption.  What a call is, beside its operands (checked by the entry points)
struct HybridCall {
    zl_curve_t curve;
    unsigned width;
    const uint64_t* init;
    size_t H, N;
    bool check;
    size_t T() const { return N * (width - 1); }
};
// host mirror: the multiplications over the pool, then the duplex call's own host path with the shared secrets as keys
template <class FrP>
int host_hybrid_encrypt(const HybridCall& c, const uint64_t* g, const uint64_t* esk, const uint64_t* pks, size_t ps, const uint64_t* headers, const uint64_t* plaintexts,
                        size_t count, uint64_t* epks, uint64_t* ciphertexts, uint64_t* tags, uint8_t* status) {
    std::vector<uint8_t> st(count, 0);
    std::vector<uint64_t> keys(count * 8);
    (void)host_mul<FrP>(pks, ps, esk, 1, count, c.check, keys.data(), st.data(), false);  // the secrets first: an item refused here ends with epk = (0, 1) as well
    (void)host_mul<FrP>(g, 0, esk, 1, count, c.check, epks, st.data(), true);
    const int rc = zl_poseidon_duplex_encrypt_batch(nullptr, c.curve, c.width, c.init, keys.data(), 2, headers, c.H, plaintexts, c.N, count, ciphertexts, tags);
    if (rc) return rc;
    bool bad = false;
    for (size_t i = 0; i < count; i++) {
        bad |= st[i] != 0;
        if (status) status[i] = st[i];
    }
    return bad && !status ? ZL_EINVAL : ZL_OK;
}
template <class FrP>
int host_hybrid_decrypt(const HybridCall& c, const uint64_t* sks, size_t ks, const uint64_t* epks, const uint64_t* headers, const uint64_t* ciphertexts, const uint64_t* tags,
                        size_t count, uint64_t* plaintexts, uint8_t* ok_each, uint8_t* status) {
    std::vector<uint8_t> st(count, 0);
    std::vector<uint64_t> keys(count * 8);
    (void)host_mul<FrP>(epks, 1, sks, ks, count, c.check, keys.data(), st.data(), false);
    const int rc = zl_poseidon_duplex_decrypt_batch(nullptr, c.curve, c.width, c.init, keys.data(), 2, headers, c.H, ciphertexts, tags, c.N, count, plaintexts, ok_each);
    if (rc) return rc;
    for (size_t i = 0; i < count; i++) {
        if (st[i]) ok_each[i] = 0;
        if (status) status[i] = st[i];
    }
    return ZL_OK;
}
// device: per chunk the ephemeral public keys (fixed-base from ZL_TUNE_ED_FIXED_MIN items), the shared secrets into the slot as m x 2 canonical elements, then
// the duplex call's device-pointer form reads them as keys with key_len = 2 -- no bus round trip, k_pos_duplex unchanged.  The statuses of the two launches merge
// on the device (`keep`): the secrets first, so an item refused there ends with epk = (0, 1) too.
template <class FrP>
int dev_hybrid_encrypt(zl_ctx* ctx, bool on_host_ptrs, const HybridCall& c, const uint64_t* g, const uint64_t* esk, const uint64_t* pks, size_t ps, const uint64_t* headers,
                       const uint64_t* plaintexts, size_t count, uint64_t* epks, uint64_t* ciphertexts, uint64_t* tags, uint8_t* status) {
    std::vector<uint32_t> fixed;
    uint8_t gst = 0;
    const bool fx = use_fixed(0, count);
    if (fx) gst = host_fixed_table<FrP>(g, c.check, fixed);
    const size_t T = c.T();
    std::vector<uint8_t> st_host(count, 0);
    std::vector<Seg> segs;
    if (on_host_ptrs) {
        segs = {staged(32, esk, nullptr), ps ? staged(64, pks, nullptr) : staged_once(64, pks), staged(c.H * 32, headers, nullptr), staged(T * 32, plaintexts, ciphertexts),
                staged(64, nullptr, epks), staged(32, nullptr, tags)};
    } else {
        segs = {device(32, esk), device(ps * 64, pks), device(c.H * 32, headers), device(T * 32, plaintexts), device(64, epks), device(32, tags)};
    }
    segs.push_back(staged(1, nullptr, st_host.data()));                      // 6: the merged statuses
    segs.push_back(staged(64, nullptr, nullptr));                            // 7: the shared secrets
    segs.push_back(staged_once(64, g));                                      // 8: the generator (host memory in every form)
    segs.push_back(staged_once(fx ? FIXED_TABLE_BYTES : 0, fixed.data()));   // 9
    segs.push_back(on_host_ptrs ? staged(0, nullptr, nullptr) : device(T * 32, ciphertexts));  // 10: where the device form writes the ciphertext
    segs.push_back(on_host_ptrs ? staged(0, nullptr, nullptr) : device(1, status));            // 11: ... and the statuses
    int rc = run_chunks(ctx, count, true, segs, [&](size_t, size_t m, void* const* d, uint32_t* tables, uint32_t* flag) -> int {
        const MulCall pub{c.check, 0, 1, fx ? static_cast<const uint32_t*>(d[9]) : nullptr, gst}, sec{c.check, ps, 1, nullptr, 0};
        int r = launch_mul<FrP>(ctx, sec, u64(d[1]), u64(d[0]), m, tables, u64(d[7]), u8(d[6]), false, flag);  // (the order of the host mirror)
        if (!r) r = launch_mul<FrP>(ctx, pub, u64(d[8]), u64(d[0]), m, tables, u64(d[4]), u8(d[6]), true, flag);
        if (r) return r;
        if (d[11]) ZL_HIP(ctx, hipMemcpyAsync(d[11], d[6], m, hipMemcpyDeviceToDevice, ctx->stream));
        return zl_poseidon_duplex_encrypt_batch_dev(ctx, c.curve, c.width, c.init, d[7], 2, d[2], c.H, d[3], c.N, m, on_host_ptrs ? d[3] : d[10], d[5]);
    });
    if (rc) return rc;
    bool bad = false;
    for (size_t i = 0; i < count; i++) bad |= st_host[i] != 0;
    if (on_host_ptrs && status) memcpy(status, st_host.data(), count);
    return bad && !status ? ZL_EINVAL : ZL_OK;
}
template <class FrP>
int dev_hybrid_decrypt(zl_ctx* ctx, bool on_host_ptrs, const HybridCall& c, const uint64_t* sks, size_t ks, const uint64_t* epks, const uint64_t* headers,
                       const uint64_t* ciphertexts, const uint64_t* tags, size_t count, uint64_t* plaintexts, uint8_t* ok_each, uint8_t* status) {
    const size_t T = c.T();
    std::vector<uint8_t> st_host(count, 0);
    std::vector<Seg> segs;
    if (on_host_ptrs) {
        segs = {ks ? staged(32, sks, nullptr) : staged_once(32, sks), staged(64, epks, nullptr), staged(c.H * 32, headers, nullptr), staged(T * 32, ciphertexts, plaintexts),
                staged(32, tags, nullptr)};
    } else {
        segs = {device(ks * 32, sks), device(64, epks), device(c.H * 32, headers), device(T * 32, ciphertexts), device(32, tags)};
    }
    segs.push_back(staged(1, nullptr, st_host.data()));  // 5: the statuses
    segs.push_back(staged(64, nullptr, nullptr));        // 6: the shared secrets
    segs.push_back(on_host_ptrs ? staged(0, nullptr, nullptr) : device(T * 32, plaintexts));  // 7
    segs.push_back(on_host_ptrs ? staged(0, nullptr, nullptr) : device(1, status));           // 8
    const int rc = run_chunks(ctx, count, true, segs, [&](size_t first, size_t m, void* const* d, uint32_t* tables, uint32_t* flag) -> int {
        const MulCall sec{c.check, 1, ks, nullptr, 0};
        const int r = launch_mul<FrP>(ctx, sec, u64(d[1]), u64(d[0]), m, tables, u64(d[6]), u8(d[5]), false, flag);
        if (r) return r;
        if (d[8]) ZL_HIP(ctx, hipMemcpyAsync(d[8], d[5], m, hipMemcpyDeviceToDevice, ctx->stream));
        return zl_poseidon_duplex_decrypt_batch_dev(ctx, c.curve, c.width, c.init, d[6], 2, d[2], c.H, d[3], d[4], c.N, m, on_host_ptrs ? d[3] : d[7], ok_each + first);
    });
    if (rc) return rc;
    for (size_t i = 0; i < count; i++) {
        if (st_host[i]) ok_each[i] = 0;
        if (on_host_ptrs && status) status[i] = st_host[i];
    }
    return ZL_OK;
}
int hybrid_params(zl_curve_t curve, unsigned width, size_t header_len, size_t blocks, unsigned flags) {
    if (!valid_curve(curve) || (flags & ~(unsigned)ZL_ED_CHECK_SUBGROUP) || zl_poseidon_duplex_permutations(width, 2, header_len, blocks) == 0) return ZL_EINVAL;
    return ZL_OK;
}
}  // namespace

#define ZL_ED_CURVE(curve, fn, ...) ((curve) == ZL_BLS12_381 ? fn<BLS12_381_Fr>(__VA_ARGS__) : fn<BN254_Fr>(__VA_ARGS__))

int zl_ed_scalar_mul_trace_rows(zl_ctx* ctx, int curve, unsigned bits, const uint64_t* points_xy, size_t point_stride, const uint64_t* scalars, size_t count, void* d_rows,
                                size_t stride_elems, uint64_t* results_out) {
    return ZL_ED_CURVE(curve, trace_run, ctx, points_xy, point_stride, scalars, true, bits, count, static_cast<uint64_t*>(d_rows), stride_elems, nullptr, results_out);
}

int zl_hybrid_encrypt_trace_rows(zl_ctx* ctx, int curve, unsigned width, unsigned bits, const uint64_t* initial_state, const uint64_t* generator_xy, const uint64_t* esk,
                                 const uint64_t* pks_xy, size_t pk_stride, const uint64_t* headers, size_t header_len, const uint64_t* plaintexts, size_t blocks, size_t count,
                                 void* d_rows, size_t stride_elems, uint64_t* epks_out, uint64_t* tags_out, uint64_t* ciphertexts_out) {
    HybridTrace c;
    const int rc = hybrid_trace_params((zl_curve_t)curve, width, bits, initial_state, generator_xy, header_len, blocks, &c);
    if (rc) return rc;
    return ZL_ED_CURVE(curve, hybrid_trace_run, ctx, c, generator_xy, esk, pks_xy, pk_stride, headers, plaintexts, true, count, static_cast<uint64_t*>(d_rows), stride_elems,
                       nullptr, epks_out, tags_out, ciphertexts_out);
}

extern "C" {

size_t zl_hybrid_encrypt_assignment_elems(zl_curve_t curve, unsigned width, unsigned bits, size_t header_len, size_t blocks) {
    return hybrid_trace_elems(curve, width, bits, header_len, blocks, nullptr);
}
int zl_hybrid_encrypt_assignments(zl_ctx* ctx, zl_curve_t curve, unsigned width, unsigned bits, const uint64_t* initial_state, const uint64_t* generator_xy, const uint64_t* esk,
                                  const uint64_t* pks_xy, size_t pk_stride, const uint64_t* headers, size_t header_len, const uint64_t* plaintexts, size_t blocks, size_t count,
                                  uint64_t* out) {
    HybridTrace c;
    const int rc = hybrid_trace_params(curve, width, bits, initial_state, generator_xy, header_len, blocks, &c);
    if (rc) return rc;
    if (pk_stride > 1 || (count && (!esk || !pks_xy || (header_len && !headers) || !plaintexts || !out))) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    if (on_host(ctx, count)) return ZL_ED_CURVE(curve, host_hybrid_trace, c, generator_xy, esk, pks_xy, pk_stride, headers, plaintexts, count, out);
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_ED_CURVE(curve, hybrid_trace_run, ctx, c, generator_xy, esk, pks_xy, pk_stride, headers, plaintexts, true, count, nullptr, 0, out, nullptr, nullptr, nullptr);
}
int zl_hybrid_encrypt_assignments_dev(zl_ctx* ctx, zl_curve_t curve, unsigned width, unsigned bits, const uint64_t* initial_state, const uint64_t* generator_xy,
                                      const void* d_esk, const void* d_pks_xy, size_t pk_stride, const void* d_headers, size_t header_len, const void* d_plaintexts,
                                      size_t blocks, size_t count, void* d_out, size_t stride_elems) {
    HybridTrace c;
    const int rc = ctx ? hybrid_trace_params(curve, width, bits, initial_state, generator_xy, header_len, blocks, &c) : ZL_EINVAL;
    if (rc) return rc;
    if (pk_stride > 1 || stride_elems < c.row.elems() || ((uintptr_t)d_out & 15) || (count && (!d_esk || !d_pks_xy || (header_len && !d_headers) || !d_plaintexts || !d_out)))
        return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_ED_CURVE(curve, hybrid_trace_run, ctx, c, generator_xy, static_cast<const uint64_t*>(d_esk), static_cast<const uint64_t*>(d_pks_xy), pk_stride,
                       static_cast<const uint64_t*>(d_headers), static_cast<const uint64_t*>(d_plaintexts), false, count, static_cast<uint64_t*>(d_out), stride_elems, nullptr,
                       nullptr, nullptr, nullptr);
}

size_t zl_ed_scalar_mul_assignment_elems(zl_curve_t curve, unsigned bits) {
    if (!valid_curve(curve)) return 0;
    return ZL_ED_CURVE(curve, trace_elems, bits);
}
int zl_ed_scalar_mul_assignments(zl_ctx* ctx, zl_curve_t curve, unsigned bits, const uint64_t* points_xy, size_t point_stride, const uint64_t* scalars, size_t count,
                                 uint64_t* out) {
    const size_t nv = zl_ed_scalar_mul_assignment_elems(curve, bits);
    if (nv == 0 || point_stride > 1 || (count && (!points_xy || !scalars || !out))) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    if (on_host(ctx, count)) return ZL_ED_CURVE(curve, host_trace, points_xy, point_stride, scalars, bits, count, out, nv);
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_ED_CURVE(curve, trace_run, ctx, points_xy, point_stride, scalars, true, bits, count, nullptr, 0, out, nullptr);
}
int zl_ed_scalar_mul_assignments_dev(zl_ctx* ctx, zl_curve_t curve, unsigned bits, const void* d_points_xy, size_t point_stride, const void* d_scalars, size_t count,
                                     void* d_out, size_t stride_elems) {
    const size_t nv = zl_ed_scalar_mul_assignment_elems(curve, bits);
    if (!ctx || nv == 0 || point_stride > 1 || stride_elems < nv || ((uintptr_t)d_out & 15) || (count && (!d_points_xy || !d_scalars || !d_out))) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_ED_CURVE(curve, trace_run, ctx, static_cast<const uint64_t*>(d_points_xy), point_stride, static_cast<const uint64_t*>(d_scalars), false, bits, count,
                       static_cast<uint64_t*>(d_out), stride_elems, nullptr, nullptr);
}

int zl_ed_params(zl_curve_t curve, uint64_t* a, uint64_t* d, uint64_t* order, uint64_t* cofactor) {
    if (!valid_curve(curve)) return ZL_EINVAL;
    return ZL_ED_CURVE(curve, params_out, a, d, order, cofactor);
}
int zl_ed_add(zl_curve_t curve, const uint64_t* p_xy, const uint64_t* q_xy, uint64_t* out_xy) {
    if (!valid_curve(curve) || !p_xy || !q_xy || !out_xy) return ZL_EINVAL;
    return ZL_ED_CURVE(curve, host_add, p_xy, q_xy, out_xy);
}
int zl_ed_scalar_mul(zl_curve_t curve, const uint64_t* p_xy, const uint64_t* k, uint64_t* out_xy) {
    if (!valid_curve(curve) || !p_xy || !k || !out_xy) return ZL_EINVAL;
    return (ZL_ED_CURVE(curve, host_item, p_xy, k, false, out_xy)) ? ZL_EINVAL : ZL_OK;
}
int zl_ed_scalar_mul_batch(zl_ctx* ctx, zl_curve_t curve, const uint64_t* points_xy, size_t point_stride, const uint64_t* scalars, size_t scalar_stride, size_t count,
                           unsigned flags, uint64_t* out_xy, uint8_t* status) {
    if (!valid_curve(curve) || point_stride > 1 || scalar_stride > 1 || (flags & ~(unsigned)ZL_ED_CHECK_SUBGROUP) || (count && (!points_xy || !scalars || !out_xy))) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    const bool check = (flags & ZL_ED_CHECK_SUBGROUP) != 0;
    if (on_host(ctx, count)) return ZL_ED_CURVE(curve, host_mul, points_xy, point_stride, scalars, scalar_stride, count, check, out_xy, status, false);
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_ED_CURVE(curve, dev_mul, ctx, true, points_xy, point_stride, scalars, scalar_stride, count, check, out_xy, status);
}
int zl_ed_scalar_mul_batch_dev(zl_ctx* ctx, zl_curve_t curve, const void* d_points_xy, size_t point_stride, const void* d_scalars, size_t scalar_stride, size_t count,
                               unsigned flags, void* d_out_xy, void* d_status) {
    if (!ctx || !valid_curve(curve) || point_stride > 1 || scalar_stride > 1 || (flags & ~(unsigned)ZL_ED_CHECK_SUBGROUP) || (count && (!d_points_xy || !d_scalars || !d_out_xy)))
        return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_ED_CURVE(curve, dev_mul, ctx, false, static_cast<const uint64_t*>(d_points_xy), point_stride, static_cast<const uint64_t*>(d_scalars), scalar_stride, count,
                       (flags & ZL_ED_CHECK_SUBGROUP) != 0, static_cast<uint64_t*>(d_out_xy), static_cast<uint8_t*>(d_status));
}

int zl_hybrid_encrypt_batch(zl_ctx* ctx, zl_curve_t curve, unsigned width, const uint64_t* initial_state, const uint64_t* generator_xy, const uint64_t* esk,
                            const uint64_t* pks_xy, size_t pk_stride, const uint64_t* headers, size_t header_len, const uint64_t* plaintexts, size_t blocks, size_t count,
                            unsigned flags, uint64_t* epks_xy, uint64_t* ciphertexts, uint64_t* tags, uint8_t* status) {
    if (hybrid_params(curve, width, header_len, blocks, flags) || pk_stride > 1) return ZL_EINVAL;
    if (count && (!generator_xy || !esk || !pks_xy || (header_len && !headers) || !plaintexts || !epks_xy || !ciphertexts || !tags)) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    const HybridCall c{curve, width, initial_state, header_len, blocks, (flags & ZL_ED_CHECK_SUBGROUP) != 0};
    if (on_host(ctx, count)) return ZL_ED_CURVE(curve, host_hybrid_encrypt, c, generator_xy, esk, pks_xy, pk_stride, headers, plaintexts, count, epks_xy, ciphertexts, tags, status);
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_ED_CURVE(curve, dev_hybrid_encrypt, ctx, true, c, generator_xy, esk, pks_xy, pk_stride, headers, plaintexts, count, epks_xy, ciphertexts, tags, status);
}
int zl_hybrid_encrypt_batch_dev(zl_ctx* ctx, zl_curve_t curve, unsigned width, const uint64_t* initial_state, const uint64_t* generator_xy, const void* d_esk,
                                const void* d_pks_xy, size_t pk_stride, const void* d_headers, size_t header_len, const void* d_plaintexts, size_t blocks, size_t count,
                                unsigned flags, void* d_epks_xy, void* d_ciphertexts, void* d_tags, void* d_status) {
    if (!ctx || hybrid_params(curve, width, header_len, blocks, flags) || pk_stride > 1) return ZL_EINVAL;
    if (count && (!generator_xy || !d_esk || !d_pks_xy || (header_len && !d_headers) || !d_plaintexts || !d_epks_xy || !d_ciphertexts || !d_tags)) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    const HybridCall c{curve, width, initial_state, header_len, blocks, (flags & ZL_ED_CHECK_SUBGROUP) != 0};
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_ED_CURVE(curve, dev_hybrid_encrypt, ctx, false, c, generator_xy, static_cast<const uint64_t*>(d_esk), static_cast<const uint64_t*>(d_pks_xy), pk_stride,
                       static_cast<const uint64_t*>(d_headers), static_cast<const uint64_t*>(d_plaintexts), count, static_cast<uint64_t*>(d_epks_xy),
                       static_cast<uint64_t*>(d_ciphertexts), static_cast<uint64_t*>(d_tags), static_cast<uint8_t*>(d_status));
}
int zl_hybrid_decrypt_batch(zl_ctx* ctx, zl_curve_t curve, unsigned width, const uint64_t* initial_state, const uint64_t* sks, size_t sk_stride, const uint64_t* epks_xy,
                            const uint64_t* headers, size_t header_len, const uint64_t* ciphertexts, const uint64_t* tags, size_t blocks, size_t count, unsigned flags,
                            uint64_t* plaintexts, uint8_t* ok_each, uint8_t* status) {
    if (hybrid_params(curve, width, header_len, blocks, flags) || sk_stride > 1) return ZL_EINVAL;
    if (count && (!sks || !epks_xy || (header_len && !headers) || !ciphertexts || !tags || !plaintexts || !ok_each)) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    const HybridCall c{curve, width, initial_state, header_len, blocks, (flags & ZL_ED_CHECK_SUBGROUP) != 0};
    if (on_host(ctx, count)) return ZL_ED_CURVE(curve, host_hybrid_decrypt, c, sks, sk_stride, epks_xy, headers, ciphertexts, tags, count, plaintexts, ok_each, status);
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_ED_CURVE(curve, dev_hybrid_decrypt, ctx, true, c, sks, sk_stride, epks_xy, headers, ciphertexts, tags, count, plaintexts, ok_each, status);
}
int zl_hybrid_decrypt_batch_dev(zl_ctx* ctx, zl_curve_t curve, unsigned width, const uint64_t* initial_state, const void* d_sks, size_t sk_stride, const void* d_epks_xy,
                                const void* d_headers, size_t header_len, const void* d_ciphertexts, const void* d_tags, size_t blocks, size_t count, unsigned flags,
                                void* d_plaintexts, uint8_t* ok_each, void* d_status) {
    if (!ctx || hybrid_params(curve, width, header_len, blocks, flags) || sk_stride > 1) return ZL_EINVAL;
    if (count && (!d_sks || !d_epks_xy || (header_len && !d_headers) || !d_ciphertexts || !d_tags || !d_plaintexts || !ok_each)) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    const HybridCall c{curve, width, initial_state, header_len, blocks, (flags & ZL_ED_CHECK_SUBGROUP) != 0};
    ZL_HIP(ctx, hipSetDevice(ctx->device));
    return ZL_ED_CURVE(curve, dev_hybrid_decrypt, ctx, false, c, static_cast<const uint64_t*>(d_sks), sk_stride, static_cast<const uint64_t*>(d_epks_xy),
                       static_cast<const uint64_t*>(d_headers), static_cast<const uint64_t*>(d_ciphertexts), static_cast<const uint64_t*>(d_tags), count,
                       static_cast<uint64_t*>(d_plaintexts), ok_each, static_cast<uint8_t*>(d_status));
}

}  // extern "C"
