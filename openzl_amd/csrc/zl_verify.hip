// zl_verify.hip -- pairings and Groth16 verification: Groth16<E>::verify, the device products of pairings, the batched verifier and their C entry points
// (include/zl_backend.h, include/zl_backend_ext.h), above the host pairing engine (zl_pairing.h) and the device Miller loops and final exponentiation
// (zl_pairing_dev.hip).  The pairing test hooks are the last section.  Host code only, no kernels; compiled by hipcc because it shares zl_field.h with them.
#include <errno.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>
#include <sys/random.h>
#include "zl_host_api.h"
#include "zl_pairing_dev.h"
#include "zl_fq12_inv.h"

using namespace openzl;

namespace {
// ---- the device Miller loops and final exponentiation of a curve (zl_pairing_dev.hip) ------------------------------------------------------------------
template <class E> struct PairDev;
template <> struct PairDev<Bls12_381> {
    static int product(zl_ctx* c, const uint64_t* p, const uint64_t* q, const uint32_t* s, size_t n, uint32_t* o) { return pairing_dev::miller_product_bls(c, p, q, s, n, o); }
    static int groups(zl_ctx* c, const uint64_t* p, const uint64_t* q, size_t n, size_t g, uint32_t* o) { return pairing_dev::miller_groups_bls(c, p, q, nullptr, n, g, o); }
    static int groups_fexp(zl_ctx* c, const uint64_t* p, const uint64_t* q, size_t n, size_t g, uint32_t* o, uint8_t* s) { return pairing_dev::pairing_groups_bls(c, p, q, nullptr, n, g, o, s); }
    static int fexp(zl_ctx* c, const uint32_t* in, size_t n, uint32_t* o, uint8_t* s) { return pairing_dev::final_exp_bls(c, in, n, o, s); }
};
template <> struct PairDev<Bn254> {
    static int product(zl_ctx* c, const uint64_t* p, const uint64_t* q, const uint32_t* s, size_t n, uint32_t* o) { return pairing_dev::miller_product_bn(c, p, q, s, n, o); }
    static int groups(zl_ctx* c, const uint64_t* p, const uint64_t* q, size_t n, size_t g, uint32_t* o) { return pairing_dev::miller_groups_bn(c, p, q, nullptr, n, g, o); }
    static int groups_fexp(zl_ctx* c, const uint64_t* p, const uint64_t* q, size_t n, size_t g, uint32_t* o, uint8_t* s) { return pairing_dev::pairing_groups_bn(c, p, q, nullptr, n, g, o, s); }
    static int fexp(zl_ctx* c, const uint32_t* in, size_t n, uint32_t* o, uint8_t* s) { return pairing_dev::final_exp_bn(c, in, n, o, s); }
};
template <class E> using EngOf = pairing::Engine<typename E::G1::FqP, typename E::PairingP>;
template <class E> using Fq12Of = typename EngOf<E>::Fq12;
template <class E> using G1Of = XYZZ<typename E::G1::F>;
template <class E> using FrOf = Fp<typename E::FrP>;
template <class E> constexpr size_t Q1 = 2 * E::G1::FQ64;  // u64 words of a G1 point; a G2 point has twice, an Fq12 value six times as many

// fn(Bls12_381{}) or fn(Bn254{})
template <class Fn>
int by_curve(int curve, Fn fn) {
    if (curve == ZL_BLS12_381) return fn(Bls12_381{});
    if (curve == ZL_BN254) return fn(Bn254{});
    return ZL_EINVAL;
}

// ---- G1 points and scalars as the C interface carries them ---------------------------------------------------------------------------------------------
// canonical affine words (x || y; all-zero = infinity)
template <class E>
G1Of<E> g1_load(const uint64_t* xy) {
    using F1 = typename E::G1::F;
    constexpr int W1 = FieldIO<F1>::WORDS;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(xy);
    uint32_t acc = 0;
    for (int k = 0; k < 2 * W1; k++) acc |= w[k];
    if (!acc) return G1Of<E>::inf();
    return G1Of<E>::from_affine(Affine<F1>{FieldIO<F1>::load_canon(w), FieldIO<F1>::load_canon(w + W1)});
}
// out = the canonical affine words of p, or of -p
template <class E>
void g1_store(G1Of<E> p, bool negate, uint64_t* out) {
    using F1 = typename E::G1::F;
    memset(out, 0, Q1<E> * 8);
    if (p.is_inf()) return;
    if (negate) zl::neg_inplace(p);
    const Affine<F1> a = zl::to_affine(p);
    uint32_t* w = reinterpret_cast<uint32_t*>(out);
    FieldIO<F1>::store_canon(w, a.x);
    FieldIO<F1>::store_canon(w + FieldIO<F1>::WORDS, a.y);
}
// The C of a proof.  Only the words are read: a caller with C at infinity passes all-zero words together with c_inf, as the decoders do.  (The device
// combination of the batch, sum_rho_c, skips the words when the flag is set; every other user of C comes through here and never looks at the flag.)
template <class E>
G1Of<E> proof_c(const zl_g16_proof& pr) { return g1_load<E>(pr.c); }
// The public-input contract of every verifying entry point: n values of 4 u64 words, each below r.  x + k r is the residue x -- the Montgomery products of the
// combination reduce it, and the 256 scalar bits of the per-proof IC walk over a point of order r -- so without this check x and x + k r would verify as one
// statement, while a caller that keys on the 32 bytes it handed over has two.  A plain word comparison, made before anything is drawn, allocated or launched;
// a call that fails it is refused whole (ZL_EINVAL, no output written), as the reference's typed field elements fail at deserialisation and as the MSM and
// the batched Poseidon entry points refuse the same kind of input.
template <class E>
bool publics_canonical(const uint64_t* pubs, size_t n) {
    using FrP = typename E::FrP;
    static_assert(FrP::N == 8, "scalar fields are 8 x 32 bits");
    for (size_t i = 0; i < n; i++) {
        const uint64_t* w = pubs + 4 * i;
        uint64_t br = 0;
        for (int j = 0; j < 8; j++) br = (((w[j / 2] >> (32 * (j % 2))) & 0xffffffffu) - FrP::mod(j) - br) >> 63;
        if (!br) return false;  // no borrow out of w - r: w >= r
    }
    return true;
}
template <class E>
FrOf<E> fr_canon(const uint64_t* w4) {
    FrOf<E> c;
    memcpy(c.l, w4, 32);
    return c;
}
// rho_i of draw_rho as a canonical scalar
template <class E>
FrOf<E> fr_rho(const std::vector<uint64_t>& rho, size_t i) {
    const uint64_t w[4] = {rho[2 * i], rho[2 * i + 1], 0, 0};
    return fr_canon<E>(w);
}
template <class E>
G1Of<E> g1_mul(const G1Of<E>& p, const FrOf<E>& k_canon) {
    uint32_t k[8];
    memcpy(k, k_canon.l, 32);
    return zl::mul_scalar(p, k);
}

// ---- the verifying key and the four pairs of a proof --------------------------------------------------------------------------------------------------
// A verifying key as canonical affine points (all-zero = infinity); gamma_abc = n_abc points, the first pairs with the constant ONE
struct BatchVk {
    const uint64_t *alpha_g1, *beta_g2, *gamma_g2, *delta_g2, *gamma_abc;
    size_t n_abc;
};
template <class E>
BatchVk batch_vk(const typename Groth16<E>::VerifyingContext& v) {
    return BatchVk{v.alpha_g1.data(), v.beta_g2.data(), v.gamma_g2.data(), v.delta_g2.data(), v.gamma_abc_g1.data(), v.gamma_abc_g1.size() / Q1<E>};
}
template <class E> const typename Groth16<E>::VerifyingContext& key_vk(const zl_g16_keys* k);
template <> const Groth16<Bls12_381>::VerifyingContext& key_vk<Bls12_381>(const zl_g16_keys* k) { return k->vk_bls; }
template <> const Groth16<Bn254>::VerifyingContext& key_vk<Bn254>(const zl_g16_keys* k) { return k->vk_bn; }
template <class E>
BatchVk batch_vk(const zl_g16_keys* k) { return batch_vk<E>(key_vk<E>(k)); }

// prepare_inputs: IC = sum_j e_j gamma_abc[j] for n_abc canonical scalars.  e_0 multiplies the constant ONE: 1 for one proof, sum_i rho_i for a combination.
template <class E>
G1Of<E> ic(const BatchVk& vk, const FrOf<E>* e) {
    G1Of<E> acc = G1Of<E>::inf();
    for (size_t j = 0; j < vk.n_abc; j++) zl::add_full(acc, g1_mul<E>(g1_load<E>(vk.gamma_abc + j * Q1<E>), e[j]));
    return acc;
}

// A launch set of m items (products of pairs) is laid out group-major: pair `pair` of item `item` sits at this index, so that pair p belongs to group p % m of the
// device launch (miller_groups_*) and group j is the product of item j.
constexpr size_t group_major(size_t pair, size_t item, size_t m) { return pair * m + item; }

// Items of `each` pairs per launch set: what MAX_PAIRS holds.  Only a knob that is SET lowers it, the tests' way to several sets at small counts:
//   * ZL_TUNE_PAIR_SET, pairs per launch set of the Miller loops (zl_pairing_dev.h), for the reject path of verify_batch_t (`products` false);
//   * ZL_TUNE_FEXP_CHUNK for zl_pairing_products (`products` true).  The knob has two meanings: it always is the number of values per k_pd_fexp launch
//     (zl_pairing_dev.hip reads it: final_exp_*, pairing_groups_*), and, when set, it also is the number of products per launch set here.
size_t items_per_set(size_t each, bool products) {
    size_t pairs = pairing_dev::MAX_PAIRS, items = pairs;
    if (products) {
        const int tune = zl_tune("ZL_TUNE_FEXP_CHUNK", 0);
        if (tune >= 1) items = (size_t)tune;
    } else {
        pairs = pairing_dev::pair_set(zl_tune("ZL_TUNE_PAIR_SET", (int)pairing_dev::MAX_PAIRS));
    }
    return std::max<size_t>(1, std::min(pairs / each, items));
}

// The four pairs of each of m proofs, e(A, B) e(-C, delta) e(-IC, gamma) e(-alpha, beta) == 1, as a group-major launch set: ps = 4 m G1 points, qs = 4 m G2 points.
// pubs: the m x (n_abc - 1) public inputs, 4 canonical u64 words each.
template <class E>
void four_pairs(const BatchVk& vk, const zl_g16_proof* proofs, const uint64_t* pubs, size_t m, uint64_t* ps, uint64_t* qs) {
    constexpr size_t q1 = Q1<E>, q2 = 2 * q1;
    const size_t n_public = vk.n_abc - 1;
    uint64_t n_alpha[q1];
    g1_store<E>(g1_load<E>(vk.alpha_g1), true, n_alpha);
    const uint64_t one[4] = {1, 0, 0, 0};
    std::vector<FrOf<E>> e(vk.n_abc, fr_canon<E>(one));
    for (size_t i = 0; i < m; i++) {
        const zl_g16_proof& pr = proofs[i];
        for (size_t j = 0; j < n_public; j++) e[j + 1] = fr_canon<E>(pubs + (i * n_public + j) * 4);
        const size_t ab = group_major(0, i, m), cd = group_major(1, i, m), ig = group_major(2, i, m), al = group_major(3, i, m);
        memcpy(ps + ab * q1, pr.a, q1 * 8);
        memcpy(qs + ab * q2, pr.b, q2 * 8);
        g1_store<E>(proof_c<E>(pr), true, ps + cd * q1);
        memcpy(qs + cd * q2, vk.delta_g2, q2 * 8);
        g1_store<E>(ic<E>(vk, e.data()), true, ps + ig * q1);
        memcpy(qs + ig * q2, vk.gamma_g2, q2 * 8);
        memcpy(ps + al * q1, n_alpha, q1 * 8);
        memcpy(qs + al * q2, vk.beta_g2, q2 * 8);
    }
}
// The product of the `each` pairings of item i of a group-major set of m items, on the host: Miller loops in lock step, one final exponentiation
template <class E>
Fq12Of<E> host_product(const uint64_t* ps, const uint64_t* qs, size_t each, size_t m, size_t i) {
    std::vector<const uint64_t*> a(each), b(each);
    for (size_t j = 0; j < each; j++) {
        a[j] = ps + group_major(j, i, m) * Q1<E>;
        b[j] = qs + group_major(j, i, m) * 2 * Q1<E>;
    }
    return EngOf<E>::multi_pairing(a, b);
}
// A or B at infinity makes a proof invalid whatever the pairings say (the product would hold trivially)
template <class E>
bool proof_holds(const zl_g16_proof& pr, const Fq12Of<E>& gt) { return !pr.a_inf && !pr.b_inf && EngOf<E>::eq(gt, EngOf<E>::one()); }
}  // namespace

namespace openzl {
template <class E>
Result<bool> Groth16<E>::verify(const VerifyingContext& vk, const Input& input, const Proof& proof) {
    Result<bool> res{false, false, Error{ZL_EINVAL}};
    const BatchVk v = batch_vk<E>(vk);
    if (v.n_abc == 0 || input.size() + 1 != v.n_abc) return res;  // ark: wrong number of public inputs -> Err(MalformedVerifyingKey)
    static_assert(sizeof(F) == 32, "the public inputs are handed on as 4 u64 words each");
    if (!publics_canonical<E>(reinterpret_cast<const uint64_t*>(input.data()), input.size())) return res;  // ark: such an input fails to deserialise
    uint64_t ps[4 * Q1<E>], qs[8 * Q1<E>];
    four_pairs<E>(v, &proof, reinterpret_cast<const uint64_t*>(input.data()), 1, ps, qs);
    res.ok = true;
    res.value = proof_holds<E>(proof, host_product<E>(ps, qs, 4, 1, 0));
    return res;
}
template Result<bool> Groth16<Bls12_381>::verify(const VerifyingContext&, const Input&, const Proof&);
template Result<bool> Groth16<Bn254>::verify(const VerifyingContext&, const Input&, const Proof&);
}  // namespace openzl

namespace {
// ---- device products of pairings ----------------------------------------------------------------------------------------------------------------------
template <class E>
int pairing_product_t(zl_ctx* ctx, const uint64_t* ps, const uint64_t* qs, const uint32_t* scalars128, size_t n, uint64_t* out12) {
    using Eng = EngOf<E>;
    Fq12Of<E> f;
    const int rc = PairDev<E>::product(ctx, ps, qs, scalars128, n, reinterpret_cast<uint32_t*>(f.c));
    if (rc) return rc;
    bool degenerate = false;
    Eng::store(out12, Eng::final_exp(f, &degenerate));
    return degenerate ? ZL_ENOTCURVE : ZL_OK;
}

// T: the smallest reject-path set of verify_batch_t whose final exponentiations run on the device (ZL_TUNE_FEXP_DEV_MIN).  Measured: the smallest power of two
// from which the device path beat the host threads in every repetition, on both curves (profiles/final_exp_bench.log, the table in DESIGN.md §4.6)
constexpr int FEXP_DEV_MIN = 128;

// zl_pairing_products: `count` independent products of `each` pairs, Miller loops and final exponentiations on the device
template <class E>
int pairing_products_t(zl_ctx* ctx, const uint64_t* ps, const uint64_t* qs, size_t count, size_t each, uint64_t* out12, int32_t* status) {
    using Eng = EngOf<E>;
    constexpr size_t q1 = Q1<E>, q2 = 2 * q1, ow = 6 * q1;
    if (each == 0) {
        for (size_t j = 0; j < count; j++) {
            Eng::store(out12 + j * ow, Eng::one());
            if (status) status[j] = ZL_OK;
        }
        return ZL_OK;
    }
    const size_t per = items_per_set(each, true);
    std::vector<Fq12Of<E>> fs(std::min(per, count));
    std::vector<uint8_t> sing(fs.size());
    std::vector<uint64_t> pp, qq;
    for (size_t first = 0; first < count; first += per) {
        const size_t m = std::min(per, count - first);
        pp.resize(m * each * q1);
        qq.resize(m * each * q2);
        for (size_t j = 0; j < m; j++)
            for (size_t i = 0; i < each; i++) {
                memcpy(&pp[group_major(i, j, m) * q1], ps + ((first + j) * each + i) * q1, q1 * 8);
                memcpy(&qq[group_major(i, j, m) * q2], qs + ((first + j) * each + i) * q2, q2 * 8);
            }
        const int rc = PairDev<E>::groups_fexp(ctx, pp.data(), qq.data(), m * each, m, reinterpret_cast<uint32_t*>(fs.data()), sing.data());
        if (rc) return rc;
        for (size_t j = 0; j < m; j++) {
            Eng::store(out12 + (first + j) * ow, fs[j]);
            if (status) status[first + j] = sing[j] ? ZL_ENOTCURVE : ZL_OK;
        }
    }
    return ZL_OK;
}

// ---- batched Groth16 verification: the steps of verify_batch_t, in its order ------------------------------------------------------------------------------
// rho_i: nonzero 128-bit scalars, two u64 words each.  With a seed they come from SplitMix64 (a zero pair is drawn again): the combination is reproducible,
// bit for bit.  Without one they come from the OS (a zero pair becomes 1).
int draw_rho(const uint64_t* seed, std::vector<uint64_t>& rho) {
    const size_t count = rho.size() / 2;
    if (seed) {
        SplitMix64 rng(*seed);
        for (size_t i = 0; i < count; i++)
            do { rho[2 * i] = rng.next(); rho[2 * i + 1] = rng.next(); } while (!rho[2 * i] && !rho[2 * i + 1]);
        return ZL_OK;
    }
    unsigned char* b = reinterpret_cast<unsigned char*>(rho.data());
    size_t got = 0;
    while (got < rho.size() * 8) {
        const ssize_t r = getrandom(b + got, rho.size() * 8 - got, 0);
        if (r < 0) {
            if (errno == EINTR) continue;
            return ZL_EINVAL;
        }
        got += (size_t)r;
    }
    for (size_t i = 0; i < count; i++)
        if (!rho[2 * i] && !rho[2 * i + 1]) rho[2 * i] = 1;
    return ZL_OK;
}

// e_j = sum_i rho_i x_ij with x_i0 = 1, canonical: the scalars of the combination's IC, and e_0 = sum_i rho_i
template <class E>
std::vector<FrOf<E>> combined_inputs(const std::vector<uint64_t>& rho, const uint64_t* pubs, size_t n_public, size_t count) {
    using Fr = FrOf<E>;
    std::vector<Fr> e(n_public + 1, Fr::zero());
    for (size_t i = 0; i < count; i++) {
        const Fr r = zl::to_mont(fr_rho<E>(rho, i));
        e[0] = zl::add(e[0], r);
        for (size_t j = 0; j < n_public; j++) e[j + 1] = zl::add(e[j + 1], zl::mul(r, zl::to_mont(fr_canon<E>(pubs + (i * n_public + j) * 4))));
    }
    for (Fr& x : e) x = zl::from_mont(x);
    return e;
}

// sum_i rho_i C_i: a device MSM, or scalar multiplications on the host (no ctx)
template <class E>
int sum_rho_c(zl_ctx* ctx, const zl_g16_proof* proofs, const std::vector<uint64_t>& rho, size_t count, G1Of<E>* sum) {
    constexpr size_t q1 = Q1<E>;
    *sum = G1Of<E>::inf();
    if (!ctx) {
        for (size_t i = 0; i < count; i++) zl::add_full(*sum, g1_mul<E>(proof_c<E>(proofs[i]), fr_rho<E>(rho, i)));
        return ZL_OK;
    }
    std::vector<uint64_t> cs(count * q1), sc(count * 4, 0);
    for (size_t i = 0; i < count; i++) {
        if (!proofs[i].c_inf) memcpy(&cs[i * q1], proofs[i].c, q1 * 8);
        sc[4 * i] = rho[2 * i];
        sc[4 * i + 1] = rho[2 * i + 1];
    }
    uint64_t h = 0, sxy[q1];
    uint8_t sinf = 0;
    int rc = zl_bases_upload(ctx, E::curve, ZL_G1, cs.data(), count, 0, -1, 0, &h);
    if (!rc) rc = zl_msm(ctx, h, 0, sc.data(), count, sxy, &sinf);
    if (h) (void)zl_bases_free(ctx, h);
    if (!rc && !sinf) *sum = g1_load<E>(sxy);
    return rc;
}

// The count + 3 pairs of the combination: (rho_i A_i, B_i), (-sum rho_i C_i, delta), (-IC, gamma), (-(sum rho_i) alpha, beta).  On the device rho_i A_i is formed
// inside the Miller loops (combined_product hands them rho), so A_i goes in as it is; the host scales it here.
template <class E>
void combined_pairs(bool device, const BatchVk& vk, const zl_g16_proof* proofs, const std::vector<uint64_t>& rho, const std::vector<FrOf<E>>& e,
                    const G1Of<E>& sum_c, size_t count, std::vector<uint64_t>& ps, std::vector<uint64_t>& qs) {
    constexpr size_t q1 = Q1<E>, q2 = 2 * q1;
    ps.assign((count + 3) * q1, 0);
    qs.assign((count + 3) * q2, 0);
    for (size_t i = 0; i < count; i++) {
        if (device) memcpy(&ps[i * q1], proofs[i].a, q1 * 8);
        else g1_store<E>(g1_mul<E>(g1_load<E>(proofs[i].a), fr_rho<E>(rho, i)), false, &ps[i * q1]);
        memcpy(&qs[i * q2], proofs[i].b, q2 * 8);
    }
    g1_store<E>(sum_c, true, &ps[count * q1]);
    memcpy(&qs[count * q2], vk.delta_g2, q2 * 8);
    g1_store<E>(ic<E>(vk, e.data()), true, &ps[(count + 1) * q1]);
    memcpy(&qs[(count + 1) * q2], vk.gamma_g2, q2 * 8);
    g1_store<E>(g1_mul<E>(g1_load<E>(vk.alpha_g1), e[0]), true, &ps[(count + 2) * q1]);
    memcpy(&qs[(count + 2) * q2], vk.beta_g2, q2 * 8);
}

// The product of those pairings: device Miller loops that scale A_i by rho_i (the three shared pairs by 1) and one final exponentiation on the host, or all on
// the host (no ctx)
template <class E>
int combined_product(zl_ctx* ctx, const std::vector<uint64_t>& ps, const std::vector<uint64_t>& qs, const std::vector<uint64_t>& rho, size_t count, Fq12Of<E>* gt) {
    const size_t np = count + 3;
    if (!ctx) {
        *gt = host_product<E>(ps.data(), qs.data(), np, 1, 0);
        return ZL_OK;
    }
    std::vector<uint32_t> sc(np * 4, 0);
    memcpy(sc.data(), rho.data(), count * 16);
    for (size_t i = count; i < np; i++) sc[4 * i] = 1;
    Fq12Of<E> f;
    const int rc = PairDev<E>::product(ctx, ps.data(), qs.data(), sc.data(), np, reinterpret_cast<uint32_t*>(f.c));
    if (!rc) *gt = EngOf<E>::final_exp(f);
    return rc;
}

// fn(i) for every i < n on min(n, 16, hardware threads) host threads, the caller's among them, which draw their items from one counter.  (Not parallel_chunks of
// zl_host.hip: ZL_HOST_THREADS would lift its cap of 16, and its chunks are fixed in advance.)
template <class Fn>
void on_host_threads(size_t n, Fn fn) {
    std::atomic<size_t> next{0};
    auto work = [&]() {
        for (size_t i; (i = next.fetch_add(1)) < n;) fn(i);
    };
    const size_t nt = std::min<size_t>(n, std::max(1u, std::min(16u, std::thread::hardware_concurrency())));
    std::vector<std::thread> th;
    for (size_t t = 1; t < nt; t++) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
}

// gt[i] = the product of the four pairings of proof i of a group-major set of m proofs.  With a ctx the Miller loops run on the device, and so do the final
// exponentiations of a set of at least dev_min proofs: the Miller values never come to the host.  (No singular flags: a zero Miller product -- points outside the
// pairing groups -- comes out as 0, which is not one: rejected, as on the host.)  A smaller set takes them on host threads.  Without a ctx all is host work.
template <class E>
int four_pair_products(zl_ctx* ctx, const uint64_t* ps, const uint64_t* qs, size_t m, size_t dev_min, Fq12Of<E>* gt) {
    uint32_t* out = reinterpret_cast<uint32_t*>(gt);
    if (!ctx) {
        on_host_threads(m, [&](size_t i) { gt[i] = host_product<E>(ps, qs, 4, m, i); });
        return ZL_OK;
    }
    if (m >= dev_min) return PairDev<E>::groups_fexp(ctx, ps, qs, 4 * m, m, out, nullptr);
    const int rc = PairDev<E>::groups(ctx, ps, qs, 4 * m, m, out);
    if (!rc) on_host_threads(m, [&](size_t i) { gt[i] = EngOf<E>::final_exp(gt[i]); });
    return rc;
}

// A rejected batch: every proof on its own, as zl_groth16_verify, one launch set of four pairs per proof at a time (the host takes one proof at a time)
template <class E>
int verify_each(zl_ctx* ctx, const BatchVk& vk, const uint64_t* pubs, const zl_g16_proof* proofs, size_t count, uint8_t* ok_each) {
    constexpr size_t q1 = Q1<E>, q2 = 2 * q1;
    const size_t per = ctx ? items_per_set(4, false) : 1, n_public = vk.n_abc - 1;
    const size_t dev_min = (size_t)std::max(1, zl_tune("ZL_TUNE_FEXP_DEV_MIN", FEXP_DEV_MIN));
    std::vector<Fq12Of<E>> gt(std::min(per, count));
    std::vector<uint64_t> ps(4 * gt.size() * q1), qs(4 * gt.size() * q2);
    for (size_t first = 0; first < count; first += per) {
        const size_t m = std::min(per, count - first);
        four_pairs<E>(vk, proofs + first, n_public ? pubs + first * n_public * 4 : nullptr, m, ps.data(), qs.data());
        const int rc = four_pair_products<E>(ctx, ps.data(), qs.data(), m, dev_min, gt.data());
        if (rc) return rc;
        for (size_t i = 0; i < m; i++) ok_each[first + i] = proof_holds<E>(proofs[first + i], gt[i]) ? 1 : 0;
    }
    return ZL_OK;
}

// Groth16::verify of `count` proofs in one random linear combination (include/zl_backend_ext.h zl_groth16_verify_batch).  ctx == NULL: everything on the host
// (the test hook).  Each step says what it does on the device.
template <class E>
int verify_batch_t(zl_ctx* ctx, const BatchVk& vk, const uint64_t* pubs, size_t n_public, const zl_g16_proof* proofs, size_t count, const uint64_t* seed,
                   int* ok, uint8_t* ok_each) {
    if (!ok || (count && !proofs) || (count && n_public && !pubs)) return ZL_EINVAL;
    if (n_public + 1 != vk.n_abc) return ZL_EINVAL;
    if (count == 0) {
        *ok = 1;
        return ZL_OK;
    }
    if (!publics_canonical<E>(pubs, count * n_public)) return ZL_EINVAL;
    std::vector<uint64_t> rho(2 * count), ps, qs;
    int rc = draw_rho(seed, rho);
    if (rc) return rc;
    const std::vector<FrOf<E>> e = combined_inputs<E>(rho, pubs, n_public, count);
    G1Of<E> sum_c;
    if ((rc = sum_rho_c<E>(ctx, proofs, rho, count, &sum_c))) return rc;
    combined_pairs<E>(ctx != nullptr, vk, proofs, rho, e, sum_c, count, ps, qs);
    Fq12Of<E> gt;
    if ((rc = combined_product<E>(ctx, ps, qs, rho, count, &gt))) return rc;
    bool any_inf = false;
    for (size_t i = 0; i < count; i++) any_inf = any_inf || proofs[i].a_inf || proofs[i].b_inf;
    *ok = !any_inf && EngOf<E>::eq(gt, EngOf<E>::one()) ? 1 : 0;
    if (!ok_each) return ZL_OK;
    if (*ok) {
        memset(ok_each, 1, count);
        return ZL_OK;
    }
    return verify_each<E>(ctx, vk, pubs, proofs, count, ok_each);
}
}  // namespace

extern "C" {
// e(P, Q) after the final exponentiation: 12 canonical Fq coefficients of the w-polynomial (tests vs the oracle)
int zl_pairing(zl_curve_t curve, const uint64_t* p_xy, const uint64_t* q_xy, uint64_t* out12) {
    if (!p_xy || !q_xy || !out12) return ZL_EINVAL;
    return by_curve(curve, [&](auto e) {
        using Eng = EngOf<decltype(e)>;
        bool degenerate = false;  // a zero Miller value (inputs that are not points of the pairing groups): ZL_ENOTCURVE instead of a made-up number
        Eng::store(out12, Eng::multi_pairing({p_xy}, {q_xy}, &degenerate));
        return degenerate ? (int)ZL_ENOTCURVE : (int)ZL_OK;
    });
}
int zl_pairing_product(zl_ctx* ctx, zl_curve_t curve, const uint64_t* ps_xy, const uint64_t* qs_xy, size_t n, uint64_t* out12) {
    if (!ctx || !out12 || (n && (!ps_xy || !qs_xy))) return ZL_EINVAL;
    return by_curve(curve, [&](auto e) { return pairing_product_t<decltype(e)>(ctx, ps_xy, qs_xy, nullptr, n, out12); });
}
int zl_pairing_products(zl_ctx* ctx, zl_curve_t curve, const uint64_t* ps_xy, const uint64_t* qs_xy, size_t count, size_t pairs_each, uint64_t* out12,
                        int32_t* status) {
    if (!ctx || (curve != ZL_BLS12_381 && curve != ZL_BN254) || pairs_each > pairing_dev::MAX_PAIRS) return ZL_EINVAL;
    if (count == 0) return ZL_OK;
    if (!out12 || (pairs_each && (!ps_xy || !qs_xy))) return ZL_EINVAL;
    return by_curve(curve, [&](auto e) { return pairing_products_t<decltype(e)>(ctx, ps_xy, qs_xy, count, pairs_each, out12, status); });
}
// Groth16::verify: public_inputs = n x 4 u64 canonical (without the leading ONE); *ok = 1 / 0
int zl_groth16_verify(const zl_g16_keys* k, const uint64_t* public_inputs, size_t n, const zl_g16_proof* proof, int* ok) {
    if (!k || !proof || !ok || (!public_inputs && n)) return ZL_EINVAL;
    return by_curve(k->curve, [&](auto e) {
        using E = decltype(e);
        typename Groth16<E>::Input in(n);
        for (size_t i = 0; i < n; i++) in[i] = fr_canon<E>(public_inputs + 4 * i);
        const auto r = Groth16<E>::verify(key_vk<E>(k), in, *proof);
        if (!r.ok) return (int)r.error.code;
        *ok = r.value ? 1 : 0;
        return (int)ZL_OK;
    });
}
int zl_groth16_verify_batch(zl_ctx* ctx, const zl_g16_keys* k, const uint64_t* public_inputs, size_t n_public, const zl_g16_proof* proofs, size_t count,
                            const uint64_t* seed, int* ok, uint8_t* ok_each) {
    if (!ctx || !k) return ZL_EINVAL;
    return by_curve(k->curve, [&](auto e) {
        using E = decltype(e);
        return verify_batch_t<E>(ctx, batch_vk<E>(k), public_inputs, n_public, proofs, count, seed, ok, ok_each);
    });
}
int zl_groth16_verify_batch_bytes(zl_ctx* ctx, const zl_g16_keys* k, const uint64_t* public_inputs, size_t n_public, const uint8_t* proofs_bytes, size_t count,
                                  const uint64_t* seed, int* ok, uint8_t* ok_each, int32_t* status) {
    if (!ctx || !k || !ok || (count && !proofs_bytes) || (count && n_public && !public_inputs)) return ZL_EINVAL;
    const size_t n_abc = k->curve == ZL_BLS12_381 ? batch_vk<Bls12_381>(k).n_abc : batch_vk<Bn254>(k).n_abc;
    if (n_public + 1 != n_abc) return ZL_EINVAL;  // before any work, as zl_groth16_verify_batch
    // every public input, ahead of the decoder and whether or not its record will decode (count == 0 reads none)
    const int canonical = by_curve(k->curve, [&](auto e) { return publics_canonical<decltype(e)>(public_inputs, count * n_public) ? (int)ZL_OK : (int)ZL_EINVAL; });
    if (canonical) return canonical;
    // decode -> host structs -> the existing combination over the proofs that decoded, with their public inputs
    std::vector<zl_g16_proof> proofs(count);
    std::vector<int32_t> st(count);
    int rc = zl_groth16_proofs_from_bytes_batch(ctx, (zl_curve_t)k->curve, proofs_bytes, count, proofs.data(), st.data());
    if (rc) return rc;
    std::vector<size_t> live;
    for (size_t i = 0; i < count; i++)
        if (st[i] == ZL_OK) live.push_back(i);
    if (live.size() != count) {
        for (size_t j = 0; j < live.size(); j++) proofs[j] = proofs[live[j]];
    }
    std::vector<uint64_t> pubs;
    const uint64_t* pp = public_inputs;
    if (live.size() != count && n_public) {
        pubs.resize(live.size() * n_public * 4);
        for (size_t j = 0; j < live.size(); j++) memcpy(&pubs[j * n_public * 4], public_inputs + live[j] * n_public * 4, n_public * 32);
        pp = pubs.data();
    }
    std::vector<uint8_t> each(ok_each ? live.size() : 0);
    int vok = 0;
    rc = zl_groth16_verify_batch(ctx, k, pp, n_public, proofs.data(), live.size(), seed, &vok, ok_each ? each.data() : nullptr);
    if (rc) return rc;
    *ok = vok && live.size() == count ? 1 : 0;
    if (ok_each) {
        memset(ok_each, 0, count);
        for (size_t j = 0; j < live.size(); j++) ok_each[live[j]] = each[j];
    }
    if (status) memcpy(status, st.data(), count * sizeof(int32_t));
    return ZL_OK;
}

// ---- TEST HOOKS (include/zl_backend_test.h): they need the templates above, so they live here and not in zl_testhooks.hip ---------------------------------
// prod_i e(P_i, Q_i) through the lock-step Miller loops that Groth16::verify uses for its four pairings
int zl_test_pairing_product(zl_curve_t curve, size_t n, const uint64_t* ps_xy, const uint64_t* qs_xy, uint64_t* out12) {
    if (!out12 || ((!ps_xy || !qs_xy) && n) || n > 64) return ZL_EINVAL;
    return by_curve(curve, [&](auto e) {
        using E = decltype(e);
        using Eng = EngOf<E>;
        std::vector<const uint64_t*> ps(n), qs(n);
        for (size_t i = 0; i < n; i++) { ps[i] = ps_xy + i * Q1<E>; qs[i] = qs_xy + i * 2 * Q1<E>; }
        bool degenerate = false;
        Eng::store(out12, Eng::multi_pairing(ps, qs, &degenerate));
        return degenerate ? (int)ZL_ENOTCURVE : (int)ZL_OK;
    });
}
int zl_test_verify_batch_host(zl_curve_t curve, const uint64_t* alpha_g1, const uint64_t* beta_g2, const uint64_t* gamma_g2, const uint64_t* delta_g2,
                              const uint64_t* gamma_abc, size_t n_public, const zl_g16_proof* proofs, const uint64_t* public_inputs, size_t count,
                              const uint64_t* seed, int* ok, uint8_t* ok_each) {
    if (!alpha_g1 || !beta_g2 || !gamma_g2 || !delta_g2 || !gamma_abc) return ZL_EINVAL;
    const BatchVk vk{alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc, n_public + 1};
    return by_curve(curve, [&](auto e) { return verify_batch_t<decltype(e)>(nullptr, vk, public_inputs, n_public, proofs, count, seed, ok, ok_each); });
}
int zl_test_miller_dev(zl_ctx* ctx, zl_curve_t curve, size_t n, const uint64_t* ps_xy, const uint64_t* qs_xy, uint64_t* out) {
    if (!ctx || (n && (!ps_xy || !qs_xy || !out)) || (curve != ZL_BLS12_381 && curve != ZL_BN254)) return ZL_EINVAL;
    return by_curve(curve, [&](auto e) {
        using E = decltype(e);
        using Fq = Fp<typename E::G1::FqP>;
        constexpr size_t q1 = Q1<E>;
        for (size_t first = 0; first < n; first += pairing_dev::MAX_PAIRS) {
            const size_t m = std::min(n - first, pairing_dev::MAX_PAIRS);
            uint64_t* o = out + first * 6 * q1;
            const int rc = PairDev<E>::groups(ctx, ps_xy + first * q1, qs_xy + first * 2 * q1, m, m, reinterpret_cast<uint32_t*>(o));
            if (rc) return rc;
            for (size_t i = 0; i < m * 12; i++) {  // Montgomery -> canonical
                Fq c;
                memcpy(c.l, o + i * q1 / 2, sizeof c.l);
                c = zl::from_mont(c);
                memcpy(o + i * q1 / 2, c.l, sizeof c.l);
            }
        }
        return (int)ZL_OK;
    });
}
int zl_test_pairing_product_scaled(zl_ctx* ctx, zl_curve_t curve, size_t n, const uint64_t* ps_xy, const uint64_t* qs_xy, const uint64_t* scalars128, uint64_t* out12) {
    if (!ctx || !out12 || (n && (!ps_xy || !qs_xy)) || (curve != ZL_BLS12_381 && curve != ZL_BN254)) return ZL_EINVAL;
    return by_curve(curve, [&](auto e) { return pairing_product_t<decltype(e)>(ctx, ps_xy, qs_xy, reinterpret_cast<const uint32_t*>(scalars128), n, out12); });
}
int zl_test_final_exp(zl_curve_t curve, const uint64_t* in12, uint64_t* out12) {
    if (!in12 || !out12) return ZL_EINVAL;
    return by_curve(curve, [&](auto e) {
        using Eng = EngOf<decltype(e)>;
        typename Eng::Fq12 f;
        for (int i = 0; i < 12; i++) {
            memcpy(f.c[i].l, reinterpret_cast<const unsigned char*>(in12) + i * sizeof(f.c[i]), sizeof(f.c[i]));
            f.c[i] = zl::to_mont(f.c[i]);
        }
        bool degenerate = false;
        Eng::store(out12, Eng::final_exp(f, &degenerate));
        return degenerate ? (int)ZL_ENOTCURVE : (int)ZL_OK;
    });
}
int zl_test_final_exp_dev(zl_ctx* ctx, zl_curve_t curve, size_t count, const uint64_t* in, uint64_t* out, uint8_t* singular) {
    if (!ctx || (count && (!in || !out)) || (curve != ZL_BLS12_381 && curve != ZL_BN254)) return ZL_EINVAL;
    return by_curve(curve, [&](auto e) {
        using E = decltype(e);
        using F = Fp<typename E::G1::FqP>;
        std::vector<F> v(count * 12);
        memcpy(static_cast<void*>(v.data()), in, v.size() * sizeof(F));
        for (auto& c : v) c = zl::to_mont(c);
        const int rc = PairDev<E>::fexp(ctx, reinterpret_cast<const uint32_t*>(v.data()), count, reinterpret_cast<uint32_t*>(v.data()), singular);
        if (rc) return rc;
        for (auto& c : v) c = zl::from_mont(c);
        memcpy(out, v.data(), v.size() * sizeof(F));
        return (int)ZL_OK;
    });
}
int zl_test_fq12_inverse(zl_curve_t curve, const uint64_t* in12, uint64_t* out12, uint8_t* singular) {
    if (!in12 || !out12 || !singular || (curve != ZL_BLS12_381 && curve != ZL_BN254)) return ZL_EINVAL;
    return by_curve(curve, [&](auto e) {
        using FqP = typename decltype(e)::G1::FqP;
        using PP = typename decltype(e)::PairingP;
        fq12inv::El<FqP> f;
        memcpy(static_cast<void*>(f.c), in12, sizeof f.c);
        for (auto& c : f.c) c = zl::to_mont(c);
        bool sing = false;
        fq12inv::El<FqP> g = fq12inv::inverse<FqP, PP>(f, &sing);
        for (auto& c : g.c) c = zl::from_mont(c);
        memcpy(out12, g.c, sizeof g.c);
        *singular = sing ? 1 : 0;
        return (int)ZL_OK;
    });
}
int zl_test_fq12_zeta(zl_curve_t curve, uint64_t* out) {
    if (!out || (curve != ZL_BLS12_381 && curve != ZL_BN254)) return ZL_EINVAL;
    return by_curve(curve, [&](auto e) {
        const auto z = zl::from_mont(fq12inv::zeta<typename decltype(e)::G1::FqP>());
        memcpy(out, z.l, sizeof z.l);
        return (int)ZL_OK;
    });
}
}  // extern "C"
