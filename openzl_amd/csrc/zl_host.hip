// zl_host.hip -- implementation of the host-side plugin mirror (zl_host.h) + its C-ABI hooks (include/zl_backend.h,
// "host mirror" section): setup, the circuits, proving, the key / point / proof wire formats.  Verification (Groth16<E>::verify and the pairing entry points) is
// zl_verify.hip.  Host code only; compiled by hipcc because it shares zl_field.h with the kernels.
#include <stdlib.h>
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include <chrono>
#include <new>
#include <atomic>
#include <thread>
#include "zl_host_api.h"
#include "zl_decode_dev.h"
#include "zl_serialize.h"

// zl_groth16.hip: the prover with the assignment in the compiler's two pieces (instance block, witness block; Montgomery limbs)
int zl_groth16_prove_split(zl_ctx* ctx, const zl_g16_pk* pk, uint64_t r1cs_handle, const uint64_t* instance, const uint64_t* witness, const uint64_t* r,
                           const uint64_t* s, zl_g16_proof* out);  // zl_groth16.hip

namespace openzl {

template <class FrP>
static void to_canon_words(uint64_t* out, const Fp<FrP>& mont) {
    const Fp<FrP> c = zl::from_mont(mont);
    memcpy(out, c.l, 32);
}

// fn(lo, hi, chunk) over [0, n) on up to 64 host threads (the setup path is O(constraints) field work: Lagrange coefficients, the
// transposed sparse products, exponent vectors; single-threaded it cost 3 s of a 4 s compile at 10^6 constraints)
template <class Fn>
static void parallel_chunks(size_t n, size_t min_chunk, Fn fn, size_t max_threads = 64) {
    if (const char* e = getenv("ZL_HOST_THREADS")) max_threads = std::max(1, atoi(e));
    size_t nt = std::min<size_t>(std::max<unsigned>(1u, std::thread::hardware_concurrency()), max_threads);
    nt = std::min(nt, std::max<size_t>(1, n / std::max<size_t>(1, min_chunk)));
    if (nt <= 1) { fn((size_t)0, n, (size_t)0); return; }
    const size_t per = (n + nt - 1) / nt;
    std::vector<std::thread> th;
    for (size_t t = 0; t < nt; t++) {
        const size_t lo = t * per, hi = std::min(n, lo + per);
        if (lo >= hi) break;
        th.emplace_back([=]() { fn(lo, hi, t); });
    }
    for (auto& x : th) x.join();
}
template <class FrP>
static Fp<FrP> pow_u64(const Fp<FrP>& a, uint64_t e) {
    const uint32_t w[2] = {(uint32_t)e, (uint32_t)(e >> 32)};
    return zl::pow_words(a, w, 64);
}

template <class FrP>
void R1CS<FrP>::replicate_rows(size_t r0, size_t r1, size_t copies, uint32_t w_from, uint32_t shift, const std::vector<F>& new_witness_values) {
    const size_t rows = r1 - r0, base = A_.size();
    witness_.insert(witness_.end(), new_witness_values.begin(), new_witness_values.end());
    A_.resize(base + rows * copies);
    B_.resize(base + rows * copies);
    C_.resize(base + rows * copies);
    parallel_chunks(rows * copies, 256, [&](size_t lo, size_t hi, size_t) {
        for (size_t i = lo; i < hi; i++) {
            const size_t j = i / rows + 1, r = r0 + i % rows;
            const uint32_t delta = (uint32_t)(j * shift);
            A_[base + i] = shifted(A_[r], w_from, delta);
            B_[base + i] = shifted(B_[r], w_from, delta);
            C_[base + i] = shifted(C_[r], w_from, delta);
        }
    }, 16);  // millions of small allocations: beyond ~16 threads the page-fault / allocator contention costs more than it buys (measured: 0.7 s at 16, 2.2 s at 64)
}

template <class FrP>
void R1csExport<FrP>::build(const R1CS<FrP>& cs) {
    const size_t nc = cs.constraint_count();
    for (int m = 0; m < 3; m++) {
        const auto& rows = cs.rows(m);
        ptr[m].assign(1, 0);
        col[m].clear();
        val[m].clear();
        ptr[m].resize(rows.size() + 1);
        size_t nnz = 0;
        for (size_t r = 0; r < rows.size(); r++) { nnz += rows[r].terms.size(); ptr[m][r + 1] = (uint32_t)nnz; }
        col[m].resize(nnz);
        val[m].resize(nnz * 4);
        uint32_t* colp = col[m].data();
        uint64_t* valp = val[m].data();
        const uint32_t* pp = ptr[m].data();
        parallel_chunks(rows.size(), 4096, [&, colp, valp, pp](size_t lo, size_t hi, size_t) {
            for (size_t r = lo; r < hi; r++) {
                size_t k = pp[r];
                // variable order: instance block then witness block; keys sort the same way (witness bit is the top bit)
                for (auto& t : rows[r].terms) {
                    colp[k] = cs.var_index(t.first);
                    to_canon_words<FrP>(valp + 4 * k, t.second);
                    k++;
                }
            }
        });
        view.row_ptr[m] = ptr[m].data();
        view.col[m] = col[m].data();
        view.val[m] = val[m].data();
    }
    const auto& inst = cs.instance_assignment();
    const auto& wit = cs.witness_assignment();
    assignment.resize((inst.size() + wit.size()) * 4);
    for (size_t i = 0; i < inst.size(); i++) to_canon_words<FrP>(&assignment[4 * i], inst[i]);
    uint64_t* asg = assignment.data() + 4 * inst.size();
    parallel_chunks(wit.size(), 8192, [&, asg](size_t lo, size_t hi, size_t) {
        for (size_t i = lo; i < hi; i++) to_canon_words<FrP>(asg + 4 * i, wit[i]);
    });
    view.n_constraints = (uint32_t)nc;
    view.n_instance = (uint32_t)inst.size();
    view.n_witness = (uint32_t)wit.size();
}

template <class FrP>
static Fp<FrP> sample_nonzero_mont(SplitMix64& rng, Fp<FrP>* canon_out) {
    for (;;) {
        Fp<FrP> c = sample_canonical<FrP>(rng);
        if (c.is_zero()) continue;
        if (canon_out) *canon_out = c;
        return zl::to_mont(c);
    }
}

// Groth16::compile -- ark_groth16::generate_random_parameters / generate_parameters (groth16.rs:427-443):
// evaluate the QAP at tau through the Lagrange coefficients, then fixed-base multiplications of the generators.  The
// fixed-base part runs on the device (zl_bases_generate); the trapdoor stays in the ProvingContext for exponent checks.
template <class E>
Result<std::pair<typename Groth16<E>::ProvingContext, typename Groth16<E>::VerifyingContext>> Groth16<E>::compile(zl_ctx* ctx, const Compiler& cs,
                                                                                                                  SplitMix64& rng, const R1csExport<FrP>* exported) {
    Result<std::pair<ProvingContext, VerifyingContext>> res{false, {}, Error{ZL_EINVAL}};
    if (!ctx) return res;
    const size_t nc = cs.constraint_count(), ni = cs.num_instance_variables(), nw = cs.secret_variable_count(), nv = ni + nw;
    unsigned log_n = 1;
    while (((size_t)1 << log_n) < nc + ni) log_n++;
    if (log_n > (unsigned)FrP::TWO_ADICITY) return res;
    const size_t N = (size_t)1 << log_n;
    Trapdoor td;
    const F alpha = sample_nonzero_mont<FrP>(rng, &td.alpha), beta = sample_nonzero_mont<FrP>(rng, &td.beta),
            gamma = sample_nonzero_mont<FrP>(rng, &td.gamma), delta = sample_nonzero_mont<FrP>(rng, &td.delta);
    F w;
    for (int i = 0; i < F::N; i++) w.l[i] = FrP::two_adic_root(i);
    for (unsigned i = log_n; i < (unsigned)FrP::TWO_ADICITY; i++) w = zl::sqr(w);
    // tau outside the domain
    F tau, zt;
    for (;;) {
        tau = sample_nonzero_mont<FrP>(rng, &td.tau);
        zt = tau;
        for (unsigned i = 0; i < log_n; i++) zt = zl::sqr(zt);
        zt = zl::sub(zt, F::one());  // Z(tau) = tau^N - 1
        if (!zt.is_zero()) break;
    }
    // Lagrange coefficients L_j = Z(tau)/N * w^j / (tau - w^j), batch inversion
    const bool dbg = getenv("ZL_DEBUG_TIMING") != nullptr;
    auto tmark = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!dbg) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[zl] compile: %-28s %.3f s\n", what, std::chrono::duration<double>(now - tmark).count());
        tmark = now;
    };
    std::vector<F> L(N), den(N), pref(N);
    {
        const F scale = zl::mul(zt, zl::inv(zl::from_u64<FrP>((uint64_t)N)));
        parallel_chunks(N, 4096, [&](size_t lo, size_t hi, size_t) {  // every chunk shares one inversion among its denominators
            F wj = pow_u64<FrP>(w, (uint64_t)lo);
            F acc = F::one();
            for (size_t j = lo; j < hi; j++) {
                den[j] = zl::sub(tau, wj);
                L[j] = wj;
                wj = zl::mul(wj, w);
                pref[j] = acc;
                acc = zl::mul(acc, den[j]);
            }
            F inv = zl::inv(acc);
            for (size_t j = hi; j-- > lo;) {
                const F dinv = zl::mul(inv, pref[j]);
                inv = zl::mul(inv, den[j]);
                L[j] = zl::mul(zl::mul(L[j], dinv), scale);
            }
        });
    }
    lap("lagrange");
    std::vector<F> u(nv, F::zero()), v(nv, F::zero()), ww(nv, F::zero());
    for (size_t j = 0; j < ni; j++) u[j] = L[nc + j];
    {
        // u = A^T L, v = B^T L, w = C^T L: scatter-adds over the variables.  Row chunks accumulate into private vectors (<= 8 per matrix),
        // which are then summed per variable range; the three matrices run side by side.
        auto transposed = [&](int m, std::vector<F>& dst) {
            const auto& rows = cs.rows(m);
            const size_t parts = std::min<size_t>(8, std::max<size_t>(1, rows.size() / 65536));
            std::vector<std::vector<F>> priv(parts > 1 ? parts - 1 : 0, std::vector<F>(nv, F::zero()));
            const size_t per = (rows.size() + parts - 1) / parts;
            std::vector<std::thread> th;
            for (size_t p = 0; p < parts; p++) {
                th.emplace_back([&, p]() {
                    std::vector<F>& acc = p == 0 ? dst : priv[p - 1];
                    const size_t lo = p * per, hi = std::min(rows.size(), lo + per);
                    for (size_t row = lo; row < hi; row++)
                        for (auto& t : rows[row].terms) {
                            const uint32_t i = cs.var_index(t.first);
                            acc[i] = zl::add(acc[i], zl::mul(t.second, L[row]));
                        }
                });
            }
            for (auto& x : th) x.join();
            if (parts > 1)
                parallel_chunks(nv, 8192, [&](size_t lo, size_t hi, size_t) {
                    for (auto& pv : priv)
                        for (size_t i = lo; i < hi; i++) dst[i] = zl::add(dst[i], pv[i]);
                });
        };
        std::thread tb([&]() { transposed(1, v); }), tc([&]() { transposed(2, ww); });
        transposed(0, u);
        tb.join();
        tc.join();
    }
    lap("transposed products");
    const F dinv = zl::inv(delta), ginv = zl::inv(gamma);
    // exponent vectors (canonical) for the device generator
    std::vector<uint64_t> ea(nv * 4), eb(nv * 4), eh((N - 1) * 4), el(std::max<size_t>(nw, 1) * 4), single(5 * 4);
    VerifyingContext vk;
    vk.gamma_abc_exponents.resize(ni);
    parallel_chunks(nv, 8192, [&](size_t lo, size_t hi, size_t) {
        for (size_t i = lo; i < hi; i++) {
            to_canon_words<FrP>(&ea[4 * i], u[i]);
            to_canon_words<FrP>(&eb[4 * i], v[i]);
            const F comb = zl::add(zl::add(zl::mul(beta, u[i]), zl::mul(alpha, v[i])), ww[i]);
            if (i < ni) vk.gamma_abc_exponents[i] = zl::mul(comb, ginv);
            else to_canon_words<FrP>(&el[4 * (i - ni)], zl::mul(comb, dinv));
        }
    });
    parallel_chunks(N - 1, 8192, [&](size_t lo, size_t hi, size_t) {
        F tp = zl::mul(zl::mul(zt, dinv), pow_u64<FrP>(tau, (uint64_t)lo));
        for (size_t j = lo; j < hi; j++) { to_canon_words<FrP>(&eh[4 * j], tp); tp = zl::mul(tp, tau); }
    });
    lap("exponent vectors");
    ProvingContext pc;
    pc.ctx = ctx;
    pc.trapdoor = td;
    pc.has_trapdoor = true;
    pc.n_instance = ni;
    pc.n_witness = nw;
    pc.domain_size = N;
    int rc = zl_bases_generate(ctx, E::curve, ZL_G1, ea.data(), nv, &pc.a_query);
    if (!rc) rc = zl_bases_generate(ctx, E::curve, ZL_G1, eb.data(), nv, &pc.b_g1_query);
    if (!rc) rc = zl_bases_generate(ctx, E::curve, ZL_G2, eb.data(), nv, &pc.b_g2_query);
    if (!rc) rc = zl_bases_generate(ctx, E::curve, ZL_G1, eh.data(), N - 1, &pc.h_query);
    if (!rc) rc = zl_bases_generate(ctx, E::curve, ZL_G1, el.data(), nw, &pc.l_query);
    lap("device generation (5 queries)");
    if (!rc) rc = build_window_tables(pc);
    lap("window tables");
    if (!rc) {
        R1csExport<FrP> own;
        if (!exported) own.build(cs);
        rc = zl_r1cs_upload(ctx, E::curve, exported ? &exported->view : &own.view, &pc.r1cs);
        pc.n_constraints = nc;
        pc.circuit_digest = cs.structure_digest();
        pc.witness_only_ok = cs.witness_only_compatible();
    }
    lap("r1cs export + upload");
    // alpha*G1, beta*G1, delta*G1, beta*G2, delta*G2
    const size_t q1 = 2 * E::G1::FQ64, q2 = 4 * E::G1::FQ64;
    pc.alpha_g1.resize(q1); pc.beta_g1.resize(q1); pc.delta_g1.resize(q1); pc.beta_g2.resize(q2); pc.delta_g2.resize(q2);
    if (!rc) {
        uint64_t k3[12];
        memcpy(k3, td.alpha.l, 32); memcpy(k3 + 4, td.beta.l, 32); memcpy(k3 + 8, td.delta.l, 32);
        uint64_t h1 = 0, h2 = 0;
        std::vector<uint64_t> tmp(3 * q2);
        rc = zl_bases_generate(ctx, E::curve, ZL_G1, k3, 3, &h1);
        if (!rc) rc = zl_bases_download(ctx, h1, 0, 3, tmp.data());
        if (!rc) {
            memcpy(pc.alpha_g1.data(), &tmp[0], q1 * 8);
            memcpy(pc.beta_g1.data(), &tmp[q1], q1 * 8);
            memcpy(pc.delta_g1.data(), &tmp[2 * q1], q1 * 8);
        }
        if (h1) (void)zl_bases_free(ctx, h1);
        if (!rc) rc = zl_bases_generate(ctx, E::curve, ZL_G2, k3 + 4, 2, &h2);
        if (!rc) rc = zl_bases_download(ctx, h2, 0, 2, tmp.data());
        if (!rc) {
            memcpy(pc.beta_g2.data(), &tmp[0], q2 * 8);
            memcpy(pc.delta_g2.data(), &tmp[q2], q2 * 8);
        }
        if (h2) (void)zl_bases_free(ctx, h2);
    }
    // verifying key: alpha G1, beta G2, gamma G2, delta G2, gamma_abc_i G1 (device fixed-base, then copied back)
    if (!rc) {
        vk.alpha_g1 = pc.alpha_g1;
        vk.beta_g2 = pc.beta_g2;
        vk.delta_g2 = pc.delta_g2;
        vk.gamma_g2.resize(q2);
        vk.gamma_abc_g1.resize(ni * q1);
        uint64_t kg[4];
        memcpy(kg, td.gamma.l, 32);
        uint64_t h = 0;
        rc = zl_bases_generate(ctx, E::curve, ZL_G2, kg, 1, &h);
        if (!rc) rc = zl_bases_download(ctx, h, 0, 1, vk.gamma_g2.data());
        if (h) (void)zl_bases_free(ctx, h);
        std::vector<uint64_t> eg(ni * 4);
        for (size_t i = 0; i < ni; i++) to_canon_words<FrP>(&eg[4 * i], vk.gamma_abc_exponents[i]);
        h = 0;
        if (!rc) rc = zl_bases_generate(ctx, E::curve, ZL_G1, eg.data(), ni, &h);
        if (!rc) rc = zl_bases_download(ctx, h, 0, ni, vk.gamma_abc_g1.data());
        if (h) (void)zl_bases_free(ctx, h);
    }
    lap("single points + vk");
    if (rc) {
        release(pc);
        res.error = Error{rc};
        return res;
    }
    res.ok = true;
    res.value = {pc, vk};
    return res;
}

// Window tables for the queries of a large proving key (static per circuit, like the key itself): the five MSMs of every proof then
// run on one merged bucket set each.  Measured at N = 2^20 (958 465 constraints): prove 33.5 -> 29.2 ms in round 1 with c = 20 for the G1
// queries (13 windows) and c = 16 for the G2 query; re-measured in round 3 (19.4 ms): G1 c = 19 / 21 -> 20.9 / 22.6 ms, G2 c = 17 / 18 / 20 -> 19.4 / 19.2 / 20.5;
// round 5 (18.1 ms, profiles/r05_g16_table_widths.log, two interleaved passes): G1 19 / 21 -> 19.4 / 20.6, G2 17 / 18 / 19 -> 18.4 / 17.9-18.35 / 19.0: the defaults stand.
// Memory: 13 x 128 B per G1 point, 16 x 256 B per G2 point (about 11 GB for this key).  Small keys stay on the plain path: a query gets its table from
// 2^19 points on (ZL_TUNE_G16_TABLE_MIN_LOG: unset, 0 or not a number = 19; any other value clamped to 1 .. 30 -- tests set it low, so that compile and
// decode build tables for small keys).
template <class E>
int Groth16<E>::build_window_tables(const ProvingContext& pc) {
    const int tuned = zl_tune("ZL_TUNE_G16_TABLE_MIN_LOG", 19);
    const int min_log = tuned == 0 ? 19 : std::clamp(tuned, 1, 30);
    const size_t big = (size_t)1 << min_log, nv = pc.n_instance + pc.n_witness;
    const char* e1 = getenv("ZL_TUNE_G1_TABLE_C");
    const char* e2 = getenv("ZL_TUNE_G2_TABLE_C");
    const int c1 = e1 ? atoi(e1) : 20, c2 = e2 ? atoi(e2) : 16;
    const struct { uint64_t h; size_t n; int c; } q[5] = {
        {pc.a_query, nv, c1}, {pc.b_g1_query, nv, c1}, {pc.h_query, pc.domain_size - 1, c1}, {pc.l_query, pc.n_witness, c1}, {pc.b_g2_query, nv, c2}};
    int rc = ZL_OK;
    for (const auto& e : q)
        if (!rc && e.n >= big) rc = zl_bases_precompute(pc.ctx, e.h, e.c);
    return rc;
}

template <class E> struct CodecOf;
template <> struct CodecOf<Bls12_381> { using type = serialize::BlsCodec; };
template <> struct CodecOf<Bn254> { using type = serialize::BnCodec; };

static void put_u64le(std::vector<uint8_t>& out, uint64_t v) {
    for (int i = 0; i < 8; i++) out.push_back((uint8_t)(v >> (8 * i)));
}
static bool all_zero_words(const uint64_t* w, size_t n) {
    uint64_t acc = 0;
    for (size_t i = 0; i < n; i++) acc |= w[i];
    return acc == 0;
}

template <class E>
std::vector<uint8_t> Groth16<E>::encode_verifying_key(const VerifyingContext& vk) {
    using C = typename CodecOf<E>::type;
    const size_t q1 = 2 * E::G1::FQ64, ni = vk.gamma_abc_g1.size() / q1;
    std::vector<uint8_t> out(C::G1_BYTES + 3 * C::G2_BYTES);
    uint8_t* p = out.data();
    C::g1_to_bytes(vk.alpha_g1.data(), all_zero_words(vk.alpha_g1.data(), q1), p); p += C::G1_BYTES;
    for (const auto* g : {&vk.beta_g2, &vk.gamma_g2, &vk.delta_g2}) { C::g2_to_bytes(g->data(), all_zero_words(g->data(), 2 * q1), p); p += C::G2_BYTES; }
    put_u64le(out, ni);
    const size_t at = out.size();
    out.resize(at + ni * C::G1_BYTES);
    for (size_t i = 0; i < ni; i++) C::g1_to_bytes(&vk.gamma_abc_g1[i * q1], all_zero_words(&vk.gamma_abc_g1[i * q1], q1), out.data() + at + i * C::G1_BYTES);
    return out;
}

template <class E>
Result<std::vector<uint8_t>> Groth16<E>::encode(const ProvingContext& pc, const VerifyingContext& vk) {
    using C = typename CodecOf<E>::type;
    Result<std::vector<uint8_t>> res{false, {}, Error{ZL_EINVAL}};
    if (!pc.ctx) return res;
    const size_t q1 = 2 * E::G1::FQ64, q2 = 2 * q1, ni = pc.n_instance, nv = pc.n_instance + pc.n_witness;
    if (vk.gamma_abc_g1.size() != ni * q1 || pc.domain_size < 2) return res;
    std::vector<uint8_t>& out = res.value;
    auto put_g1 = [&](const uint64_t* xy) { const size_t at = out.size(); out.resize(at + C::G1_UNC_BYTES); C::g1_to_uncompressed(xy, all_zero_words(xy, q1), out.data() + at); };
    auto put_g2 = [&](const uint64_t* xy) { const size_t at = out.size(); out.resize(at + C::G2_UNC_BYTES); C::g2_to_uncompressed(xy, all_zero_words(xy, q2), out.data() + at); };
    // vk
    put_g1(vk.alpha_g1.data()); put_g2(vk.beta_g2.data()); put_g2(vk.gamma_g2.data()); put_g2(vk.delta_g2.data());
    put_u64le(out, ni);
    for (size_t i = 0; i < ni; i++) put_g1(&vk.gamma_abc_g1[i * q1]);
    put_g1(pc.beta_g1.data()); put_g1(pc.delta_g1.data());
    // the five queries: downloaded as canonical affine words, re-encoded in place (only infinity records differ from the raw words)
    const struct { uint64_t h; size_t n; bool g2; } q[5] = {
        {pc.a_query, nv, false}, {pc.b_g1_query, nv, false}, {pc.b_g2_query, nv, true}, {pc.h_query, pc.domain_size - 1, false}, {pc.l_query, pc.n_witness, false}};
    for (const auto& e : q) {
        put_u64le(out, e.n);
        const size_t rec = e.g2 ? C::G2_UNC_BYTES : C::G1_UNC_BYTES, words = rec / 8, at = out.size();
        out.resize(at + e.n * rec);
        if (!e.n) continue;
        std::vector<uint64_t> tmp(e.n * words);
        const int rc = zl_bases_download(pc.ctx, e.h, 0, e.n, tmp.data());
        if (rc) { res.error = Error{rc}; res.value.clear(); return res; }
        uint8_t* base = out.data() + at;
        parallel_chunks(e.n, 16384, [&](size_t lo, size_t hi, size_t) {
            for (size_t i = lo; i < hi; i++) {
                const uint64_t* xy = &tmp[i * words];
                if (e.g2) C::g2_to_uncompressed(xy, all_zero_words(xy, words), base + i * rec);
                else C::g1_to_uncompressed(xy, all_zero_words(xy, words), base + i * rec);
            }
        });
    }
    res.ok = true;
    return res;
}

template <class E>
Result<std::pair<typename Groth16<E>::ProvingContext, typename Groth16<E>::VerifyingContext>> Groth16<E>::decode(zl_ctx* ctx, const uint8_t* in, size_t len,
                                                                                                                   unsigned flags) {
    using C = typename CodecOf<E>::type;
    Result<std::pair<ProvingContext, VerifyingContext>> res{false, {}, Error{ZL_EINVAL}};
    if (!in) return res;  // ctx == nullptr: PARSE ONLY (zl_groth16_keys_parse) -- every byte is read and validated exactly as below, nothing goes to a device
    const size_t q1 = 2 * E::G1::FQ64, q2 = 2 * q1;
    const bool check = (flags & ZL_CHECK) != 0;
    size_t pos = 0;
    int rc = ZL_OK;
    auto take = [&](size_t n) -> const uint8_t* {  // nullptr: the input ends early
        if (rc || n > len - pos) { if (!rc) rc = ZL_EINVAL; return nullptr; }
        const uint8_t* p = in + pos;
        pos += n;
        return p;
    };
    auto get_g1 = [&](std::vector<uint64_t>& xy) {
        xy.assign(q1, 0);
        uint8_t inf = 0;
        if (const uint8_t* p = take(C::G1_UNC_BYTES)) rc = C::g1_from_uncompressed(p, check, xy.data(), &inf);
    };
    auto get_g2 = [&](std::vector<uint64_t>& xy) {
        xy.assign(q2, 0);
        uint8_t inf = 0;
        if (const uint8_t* p = take(C::G2_UNC_BYTES)) rc = C::g2_from_uncompressed(p, check, xy.data(), &inf);
    };
    auto get_len = [&](size_t rec) -> size_t {  // Vec<T> length prefix, bounded by what the remaining input can hold
        const uint8_t* p = take(8);
        if (!p) return 0;
        uint64_t v = 0;
        for (int i = 0; i < 8; i++) v |= (uint64_t)p[i] << (8 * i);
        if (v > (len - pos) / rec) { rc = ZL_EINVAL; return 0; }
        return (size_t)v;
    };
    ProvingContext& pc = res.value.first;
    VerifyingContext& vk = res.value.second;
    pc.ctx = ctx;
    get_g1(vk.alpha_g1); get_g2(vk.beta_g2); get_g2(vk.gamma_g2); get_g2(vk.delta_g2);
    const size_t ni = get_len(C::G1_UNC_BYTES);
    vk.gamma_abc_g1.assign(ni * q1, 0);
    for (size_t i = 0; i < ni && !rc; i++) {
        std::vector<uint64_t> t;
        get_g1(t);
        memcpy(&vk.gamma_abc_g1[i * q1], t.data(), q1 * 8);
    }
    get_g1(pc.beta_g1); get_g1(pc.delta_g1);
    pc.alpha_g1 = vk.alpha_g1;
    pc.beta_g2 = vk.beta_g2;
    pc.delta_g2 = vk.delta_g2;
    // the five queries: validated and converted to the all-zero infinity encoding on the host, then uploaded
    size_t count[5] = {0, 0, 0, 0, 0};
    uint64_t* handle[5] = {&pc.a_query, &pc.b_g1_query, &pc.b_g2_query, &pc.h_query, &pc.l_query};
    for (int k = 0; k < 5 && !rc; k++) {
        const bool g2 = k == 2;
        const size_t rec = g2 ? C::G2_UNC_BYTES : C::G1_UNC_BYTES, words = rec / 8;
        const size_t n = count[k] = get_len(rec);
        const uint8_t* p = take(n * rec);
        if (rc) break;
        if (n == 0) continue;  // an empty query (a circuit without witnesses) has no handle; prove() never reads it
        std::vector<uint64_t> xy(n * words);
        std::atomic<int> bad{ZL_OK};
        parallel_chunks(n, 16384, [&](size_t lo, size_t hi, size_t) {
            for (size_t i = lo; i < hi; i++) {
                uint8_t inf = 0;
                // subgroup membership on the host would cost a scalar multiplication per point: with ZL_CHECK the device verifies the
                // curve equation of every uploaded point instead (zl_bases_upload)
                const int r = g2 ? C::g2_from_uncompressed(p + i * rec, false, &xy[i * words], &inf) : C::g1_from_uncompressed(p + i * rec, false, &xy[i * words], &inf);
                if (r) bad.store(r);
            }
        });
        if ((rc = bad.load())) break;
        if (ctx) rc = zl_bases_upload(ctx, E::curve, g2 ? ZL_G2 : ZL_G1, xy.data(), n, 0, -1, ZL_CANON | (check ? ZL_CHECK : 0u), handle[k]);
    }
    if (!rc && pos != len) rc = ZL_EINVAL;  // trailing bytes
    // shape: a, b1, b2 cover every variable; h has N - 1 entries for a power-of-two domain N >= 2; l covers the witnesses
    if (!rc) {
        const size_t nv = count[0], N = count[3] + 1;
        if (ni < 1 || nv < ni || count[1] != nv || count[2] != nv || count[4] != nv - ni || N < 2 || (N & (N - 1))) rc = ZL_EINVAL;
        pc.n_instance = ni;
        pc.n_witness = nv - ni;
        pc.domain_size = N;
    }
    if (!rc && ctx) rc = build_window_tables(pc);
    if (rc) {
        release(pc);
        res.value = {};
        res.error = Error{rc};
        return res;
    }
    res.ok = true;
    return res;
}

template <class E>
void Groth16<E>::release(ProvingContext& pc) {
    if (!pc.ctx) return;
    // a handle whose free is REFUSED (a fork the caller made still lives: ZL_EINVAL) stays in the context, so that a later release -- or zl_ctx_destroy --
    // still finds it (zeroing it leaked the device-resident key)
    for (uint64_t* h : {&pc.a_query, &pc.b_g1_query, &pc.b_g2_query, &pc.h_query, &pc.l_query})
        if (*h && zl_bases_free(pc.ctx, *h) != ZL_EINVAL) *h = 0;
    if (pc.r1cs && zl_r1cs_free(pc.ctx, pc.r1cs) != ZL_EINVAL) pc.r1cs = 0;
}

// Groth16::prove (groth16.rs:445-457): r, s <- rng; create_proof_with_assignment on the device
template <class E>
Result<typename Groth16<E>::Proof> Groth16<E>::prove(const ProvingContext& pc, const Compiler& cs, SplitMix64& rng, F* r_out, F* s_out, zl_ctx* lane) {
    Result<Proof> res{false, {}, Error{ZL_EINVAL}};
    if (!lane) lane = pc.ctx;
    if (lane != pc.ctx && (lane->parent != pc.ctx || !pc.r1cs)) return res;  // not a lane of this context / binding happens on the context's own ctx
    if (cs.mode() == Compiler::Mode::Setup) return res;  // the reference panics when a setup-mode compiler reaches prove
    if (cs.num_instance_variables() != pc.n_instance || cs.secret_variable_count() != pc.n_witness) return res;
    if (cs.witness_only() && !pc.r1cs) return res;  // a witness-only compiler has no rows to bind an unbound context to
    if (cs.witness_only() && !pc.witness_only_ok) return res;  // the bound circuit allocates witnesses differently without its rows (R1CS::mul)
    const F r = sample_canonical<FrP>(rng), s = sample_canonical<FrP>(rng);
    if (r_out) *r_out = r;
    if (s_out) *s_out = s;
    if (pc.r1cs && !cs.witness_only() && (cs.constraint_count() != pc.n_constraints || cs.structure_digest() != pc.circuit_digest)) return res;  // not the bound circuit
    if (!pc.r1cs) {
        // a context decoded from bytes (Groth16::decode) does not know its circuit: the first proof uploads the matrices, after checking
        // that the compiler's evaluation domain is the one the key's h_query was generated for
        const size_t nc = cs.constraint_count();
        size_t N = 2;
        while (N < nc + pc.n_instance) N <<= 1;
        if (N != pc.domain_size) return res;
        R1csExport<FrP> ex;
        ex.build(cs);
        const int rc_up = zl_r1cs_upload(pc.ctx, E::curve, &ex.view, &pc.r1cs);
        if (rc_up) { res.error = Error{rc_up}; return res; }
        pc.n_constraints = nc;
        pc.circuit_digest = cs.structure_digest();
        pc.witness_only_ok = cs.witness_only_compatible();
    }
    // only the assignment travels per proof; the matrices and the proving key are device-resident.  It goes to the device straight from the
    // compiler's two vectors (Montgomery limbs as held): no host-side concatenation
    const auto& inst = cs.instance_assignment();
    const auto& wit = cs.witness_assignment();
    zl_g16_pk pk{};
    pk.curve = E::curve;
    pk.a_query = pc.a_query; pk.b_g1_query = pc.b_g1_query; pk.h_query = pc.h_query; pk.l_query = pc.l_query; pk.b_g2_query = pc.b_g2_query;
    pk.alpha_g1 = pc.alpha_g1.data(); pk.beta_g1 = pc.beta_g1.data(); pk.delta_g1 = pc.delta_g1.data();
    pk.beta_g2 = pc.beta_g2.data(); pk.delta_g2 = pc.delta_g2.data();
    uint64_t rw[4], sw[4];
    memcpy(rw, r.l, 32);
    memcpy(sw, s.l, 32);
    const int rc = zl_groth16_prove_split(lane, &pk, pc.r1cs, reinterpret_cast<const uint64_t*>(inst.data()),
                                          wit.empty() ? nullptr : reinterpret_cast<const uint64_t*>(wit.data()), rw, sw, &res.value);
    if (rc) { res.error = Error{rc}; return res; }  // .map_err(|_| Error) groth16.rs:456
    res.ok = true;
    return res;
}

template struct Groth16<Bls12_381>;
template struct Groth16<Bn254>;
template struct R1csExport<BLS12_381_Fr>;
template struct R1csExport<BN254_Fr>;

// config 5 circuit: h_1 = H(x0, x1), h_{j+1} = H(h_j, x1), public input h_k  
// the same circuit code run by a witness-only compiler (R1CS::for_witness): every link through the gadget, values only
template <class FrP>
static R1CS<FrP> poseidon_chain_witness(uint32_t k, const Fp<FrP>& x0_canon, const Fp<FrP>& x1_canon) {
    static const poseidon::Constants<FrP> consts;
    R1CS<FrP> cs = R1CS<FrP>::for_witness();
    FpVar<FrP> cur = cs.new_witness(zl::to_mont(x0_canon));
    const FpVar<FrP> b = cs.new_witness(zl::to_mont(x1_canon));
    for (uint32_t j = 0; j < k; j++) cur = poseidon::hash(consts, cur, b, cs);
    // the public input is the chain's output (the instance block is its own vector: allocating it last changes no index)
    const FpVar<FrP> out_pub = cs.new_input(cur.value);
    cs.enforce_equal(cur, out_pub);
    return cs;
}
template <class FrP>
static R1CS<FrP> poseidon_chain(uint32_t k, const Fp<FrP>& x0_canon, const Fp<FrP>& x1_canon) {
    using F = Fp<FrP>;
    static const poseidon::Constants<FrP> consts;
    R1CS<FrP> cs = R1CS<FrP>::for_proofs();
    // expected output natively (public input is allocated first so that the instance block precedes the witnesses)
    F h = zl::to_mont(x0_canon);
    const F x1 = zl::to_mont(x1_canon);
    for (uint32_t j = 0; j < k; j++) {
        F st[3] = {zl::from_u64<FrP>(3), h, x1};
        poseidon::permute_native(consts, st);
        h = st[0];
    }
    FpVar<FrP> out_pub = cs.new_input(h);
    FpVar<FrP> a = cs.new_witness(zl::to_mont(x0_canon));
    FpVar<FrP> b = cs.new_witness(x1);
    FpVar<FrP> cur = a;
    // Links 1 and 2 are synthesised symbolically (link 1 takes a plain variable, every later link the previous link's output combination);
    // links 3.. are copies of link 2's constraints with the witness indices shifted by one link each, their witness values recomputed
    // natively.  Same circuit as k symbolic syntheses (the linear-combination arithmetic of a link is ~10^4 field multiplications and
    // was 2.5 s of host time at k = 4096).
    const uint32_t sym = k < 2 ? k : 2;
    const auto t0 = std::chrono::steady_clock::now();
    size_t rows0 = 0, wit0 = 0;
    F hv = zl::to_mont(x0_canon);
    for (uint32_t j = 0; j < sym; j++) {
        rows0 = cs.constraint_count();
        wit0 = cs.secret_variable_count();
        cur = poseidon::hash(consts, cur, b, cs);
        hv = cur.value;
    }
    const auto tA = std::chrono::steady_clock::now();
    if (getenv("ZL_DEBUG_TIMING")) fprintf(stderr, "[zl] chain: native chain + 2 symbolic links %.3f s\n", std::chrono::duration<double>(tA - t0).count());
    if (k > sym) {
        const size_t rows1 = cs.constraint_count(), per_link = cs.secret_variable_count() - wit0, copies = k - sym;
        std::vector<F> vals;
        vals.reserve(per_link * copies);
        for (size_t j = 0; j < copies; j++) {
            F st[3] = {zl::from_u64<FrP>(3), hv, x1};
            poseidon::permute_native_record(consts, st, vals);
            hv = st[0];
        }
        const auto tB = std::chrono::steady_clock::now();
        // every witness of links 1 and 2 (index >= 2: after x0, x1) moves with the copy; the instance block, x0 and x1 stay
        cs.replicate_rows(rows0, rows1, copies, 2, (uint32_t)per_link, vals);
        if (getenv("ZL_DEBUG_TIMING"))
            fprintf(stderr, "[zl] chain: native values %.3f s, replicate %.3f s\n", std::chrono::duration<double>(tB - tA).count(),
                    std::chrono::duration<double>(std::chrono::steady_clock::now() - tB).count());
        cur.lc = R1CS<FrP>::shifted(cur.lc, 2, (uint32_t)(copies * per_link));
        cur.value = hv;
    }
    cs.enforce_equal(cur, out_pub);
    return cs;
}

// Merkle membership (the reference's PathVar::verify_digest with the digest itself as the leaf, openzl-crypto/src/merkle_tree/path.rs:942-1126): the fold of
// `depth` siblings over the leaf equals the public root.  Per level, in this order: the sibling, the Boolean index bit, left = select(b, sib, cur),
// right = select(b, cur, sib) (ConditionalSwap as two conditionally_selects, plugins/arkworks/src/constraint/mod.rs:354-390), cur = H(left, right).  The
// allocation is LEVEL-major (the reference allocates all bits, then all digests, up front) so that a device lane writes its assignment row front to back
// (k_pos_merkle_trace); every hash takes two plain witnesses, so every level has the same 238 witnesses and 237 rows.
// the levels over a running digest the caller made: a witness (the leaf of poseidon_merkle) or a linear combination (the leaf hash of poseidon_merkle_leaf)
template <class FrP>
static FpVar<FrP> merkle_levels_over(R1CS<FrP>& cs, FpVar<FrP> cur, unsigned depth, uint64_t index, const Fp<FrP>* path_canon) {
    static const poseidon::Constants<FrP> consts;
    for (unsigned j = 0; j < depth; j++) {
        const FpVar<FrP> sib = cs.new_witness(zl::to_mont(path_canon[j]));
        const FpVar<FrP> b = cs.new_boolean_witness((index >> j) & 1);
        const FpVar<FrP> left = cs.select(b, sib, cur);
        const FpVar<FrP> right = cs.select(b, cur, sib);
        cur = poseidon::hash(consts, left, right, cs);
    }
    return cur;
}
template <class FrP>
static FpVar<FrP> merkle_levels(R1CS<FrP>& cs, unsigned depth, const Fp<FrP>& leaf_canon, uint64_t index, const Fp<FrP>* path_canon) {
    return merkle_levels_over(cs, cs.new_witness(zl::to_mont(leaf_canon)), depth, index, path_canon);
}
template <class FrP>
static R1CS<FrP> poseidon_merkle_witness(unsigned depth, const Fp<FrP>& leaf_canon, uint64_t index, const Fp<FrP>* path_canon) {
    R1CS<FrP> cs = R1CS<FrP>::for_witness();
    const FpVar<FrP> cur = merkle_levels(cs, depth, leaf_canon, index, path_canon);
    const FpVar<FrP> root = cs.new_input(cur.value);  // (the instance block is its own vector: allocating it last changes no index)
    cs.enforce_equal(cur, root);
    return cs;
}
template <class FrP>
static R1CS<FrP> poseidon_merkle(unsigned depth, const Fp<FrP>& leaf_canon, uint64_t index, const Fp<FrP>* path_canon) {
    using F = Fp<FrP>;
    static const poseidon::Constants<FrP> consts;
    R1CS<FrP> cs = R1CS<FrP>::for_proofs();
    // the fold's value natively: the public input is allocated first, as the chain's h_k
    F h = zl::to_mont(leaf_canon);
    for (unsigned j = 0; j < depth; j++) {
        const F sib = zl::to_mont(path_canon[j]);
        const bool right = (index >> j) & 1;
        F st[3] = {zl::from_u64<FrP>(3), right ? sib : h, right ? h : sib};
        poseidon::permute_native(consts, st);
        h = st[0];
    }
    const FpVar<FrP> root = cs.new_input(h);
    // every level is synthesised symbolically: depth <= 40 levels of ~10^4 field multiplications each
    const FpVar<FrP> cur = merkle_levels(cs, depth, leaf_canon, index, path_canon);
    cs.enforce_equal(cur, root);
    return cs;
}

// One hash of W - 1 inputs (the reference's Spec<F, ARITY> at arity 2..5): public input the digest, witnesses the inputs and the hash's S-box records.  With
// depth > 0 the digest is the LEAF of a Merkle membership instead (the reference's PathVar::verify: parameters.digest_with(leaf), then verify_digest,
// openzl-crypto/src/merkle_tree/path.rs:1109-1125): it stays a linear combination -- nothing is allocated for it, as for h_j inside a chain -- and the
// levels of poseidon_merkle fold the path over it; the public input is then the root.  One function for the full and the witness-only compiler: the full
// one allocates its public input first (the value computed natively), the witness-only one last, as the chain and the membership do.
template <class FrP, int W>
static R1CS<FrP> poseidon_arity(bool witness_only, const Fp<FrP>* in_canon, unsigned depth, uint64_t index, const Fp<FrP>* path_canon) {
    using F = Fp<FrP>;
    static const poseidon::Constants<FrP, W> consts;
    static const poseidon::Constants<FrP> consts2;
    R1CS<FrP> cs = witness_only ? R1CS<FrP>::for_witness() : R1CS<FrP>::for_proofs();
    FpVar<FrP> pub;
    if (!witness_only) {
        F st[W];
        st[0] = zl::from_u64<FrP>(consts.SPEC.tag);
        for (int i = 1; i < W; i++) st[i] = zl::to_mont(in_canon[i - 1]);
        poseidon::permute_native(consts, st);
        F h = st[0];
        for (unsigned j = 0; j < depth; j++) {
            const F sib = zl::to_mont(path_canon[j]);
            const bool right = (index >> j) & 1;
            F lv[3] = {zl::from_u64<FrP>(3), right ? sib : h, right ? h : sib};
            poseidon::permute_native(consts2, lv);
            h = lv[0];
        }
        pub = cs.new_input(h);
    }
    FpVar<FrP> in[W - 1];
    for (int i = 0; i < W - 1; i++) in[i] = cs.new_witness(zl::to_mont(in_canon[i]));
    FpVar<FrP> cur = poseidon::hash<FrP, W>(consts, in, cs);
    if (depth) cur = merkle_levels_over(cs, cur, depth, index, path_canon);
    if (witness_only) pub = cs.new_input(cur.value);
    cs.enforce_equal(cur, pub);
    return cs;
}

// The duplex cipher in circuit (poseidon::duplex_encrypt is its native form): "the public ciphertext and tag are the encryption, under a secret key and the
// public header, of a secret plaintext".  The initial state and the padding are constants; additions into the rate are linear and allocate nothing; the
// compiler's constant folding decides which S-boxes of the first permutation exist (lane 0 of round 0 and every rate lane without a key element fold).
// Public inputs: the tag, the blocks x rate ciphertext elements (Ciphertext::extend: tag, then message), the header.  Witnesses: the key, the plaintext, then
// the S-box records of the permutations in execution order.  Rows: the records', then tag = public tag, then one row per ciphertext element.  The full
// compiler allocates its public inputs first (the native values), the witness-only one last, as the other circuits do.  All inputs canonical, below r.
template <class FrP, int W>
static R1CS<FrP> poseidon_encrypt(bool witness_only, const Fp<FrP>* init_canon, const Fp<FrP>* key_canon, size_t key_len, const Fp<FrP>* header_canon, size_t header_len,
                                  const Fp<FrP>* text_canon, size_t blocks) {
    using F = Fp<FrP>;
    using V = FpVar<FrP>;
    static const poseidon::Constants<FrP, W> consts;
    constexpr size_t rate = W - 1;
    const size_t n_text = blocks * rate;
    std::vector<F> key(key_len), header(header_len), text(n_text);
    for (size_t i = 0; i < key_len; i++) key[i] = zl::to_mont(key_canon[i]);
    for (size_t i = 0; i < header_len; i++) header[i] = zl::to_mont(header_canon[i]);
    for (size_t i = 0; i < n_text; i++) text[i] = zl::to_mont(text_canon[i]);
    R1CS<FrP> cs = witness_only ? R1CS<FrP>::for_witness() : R1CS<FrP>::for_proofs();
    V pub_tag;
    std::vector<V> pub_ct(n_text), hv(header_len);
    if (!witness_only) {
        F st[W];
        for (int i = 0; i < W; i++) st[i] = zl::to_mont(init_canon[i]);
        std::vector<F> ct = text;
        pub_tag = cs.new_input(poseidon::duplex_encrypt<FrP, W>(consts, st, key.data(), key_len, header.data(), header_len, ct.data(), blocks));
        for (size_t i = 0; i < n_text; i++) pub_ct[i] = cs.new_input(ct[i]);
        for (size_t i = 0; i < header_len; i++) hv[i] = cs.new_input(header[i]);
    }
    std::vector<V> kv(key_len), pv(n_text), cv(n_text);
    for (size_t i = 0; i < key_len; i++) kv[i] = cs.new_witness(key[i]);
    for (size_t i = 0; i < n_text; i++) pv[i] = cs.new_witness(text[i]);
    // (a witness-only compiler keeps no linear combinations, so the header's VALUES can enter the state before its variables exist)
    if (witness_only)
        for (size_t i = 0; i < header_len; i++) hv[i] = V{typename R1CS<FrP>::LC{}, header[i], false};
    V state[W];
    for (int i = 0; i < W; i++) state[i] = cs.constant(zl::to_mont(init_canon[i]));
    poseidon::duplex_encrypt_circuit<FrP, W>(consts, state, kv, hv, pv, cv, cs);
    if (witness_only) {
        pub_tag = cs.new_input(state[1].value);
        for (size_t i = 0; i < n_text; i++) pub_ct[i] = cs.new_input(cv[i].value);
        for (size_t i = 0; i < header_len; i++) cs.new_input(header[i]);
    }
    cs.enforce_equal(state[1], pub_tag);
    for (size_t i = 0; i < n_text; i++) cs.enforce_equal(cv[i], pub_ct[i]);
    return cs;
}

// "Q = s P on the embedded curve, for a secret scalar s": the gadget of zl_host.h (edwards::scalar_mul_le) behind four public inputs P.x, P.y, Q.x, Q.y.
// Witnesses: s, its `bits` Boolean witnesses b_0 .. (least significant first), then what the gadget allocates: the two first selects and 13 records a step.
// Rows: the bits' Booleanity, sum 2^i b_i = s, the gadget's, Q.x and Q.y bound last.  P is NOT checked to be on the curve: it is public, the verifier checks it.
// Shape: n_witness = 1 + bits + 2 + 13 (bits - 1) = 14 bits - 10; n_constraints = bits + 1 + 2 + 13 (bits - 1) + 2 = 14 bits - 8; n_instance = 5.  Both
// compilers allocate the public inputs first: Q is known before the circuit runs (the caller computed it natively).  p, q canonical and below r; s below 2^bits.
template <class FrP>
static R1CS<FrP> ed_scalar_mul_circuit(bool witness_only, unsigned bits, const Fp<FrP>* p_canon, const uint64_t* s_words, const Fp<FrP>* q_canon, const Fp<FrP>& a_canon,
                                       const Fp<FrP>& d_canon) {
    using F = Fp<FrP>;
    using V = FpVar<FrP>;
    R1CS<FrP> cs = witness_only ? R1CS<FrP>::for_witness() : R1CS<FrP>::for_proofs();
    const edwards::Coeffs<FrP> k{zl::to_mont(a_canon), zl::to_mont(d_canon)};
    const edwards::PointVar<FrP> p{cs.new_input(zl::to_mont(p_canon[0])), cs.new_input(zl::to_mont(p_canon[1]))};
    const V qx = cs.new_input(zl::to_mont(q_canon[0])), qy = cs.new_input(zl::to_mont(q_canon[1]));
    F s_canon;
    memcpy(s_canon.l, s_words, 32);
    const V s = cs.new_witness(zl::to_mont(s_canon));
    const std::vector<V> b = edwards::scalar_bits(s, s_words, bits, cs);
    const edwards::PointVar<FrP> r = edwards::scalar_mul_le(k, p, b, cs);
    cs.enforce_equal(r.x, qx);
    cs.enforce_equal(r.y, qy);
    return cs;
}

// Hybrid<DiffieHellman, FixedDuplexer>::encrypt in circuit (openzl-crypto/src/encryption/hybrid.rs, impl Encrypt): "this ciphertext is the hybrid encryption,
// to the public key pk, of a plaintext I know" -- epk = esk G, S = esk pk, then the duplex cipher under the key (S.x, S.y): the two gadgets above joined, so
// that the cipher's key IS the agreement's output (two separate proofs would not bind them).
// Public inputs (Ciphertext::extend: epk, then tag, then message): G.x G.y pk.x pk.y epk.x epk.y tag, the N rate ciphertext elements, the H header elements.
// Witnesses: esk; its `bits` Boolean witnesses, allocated ONCE and shared by both ladders; the ladder over G (R_1 and 13 records a step); the ladder over pk in
// the same form -- its last R is S, bound to nothing public; the N rate plaintext elements; the 3 S records of the cipher as poseidon_encrypt orders them at
// K = 2.  Rows: the bits', sum 2^i b_i = esk, the G ladder's, epk.x and epk.y bound, the pk ladder's, the cipher's records, tag = public tag, one per ciphertext
// element.  G and pk are public variables and not checked to be on the curve: the verifier checks them.
// Shape, derived again (T = N rate, L = 2 + 13 (bits - 1) = 13 bits - 11 per ladder):
//   n_instance    = 1 + 2 + 2 + 2 + 1 + T + H                       = 8 + T + H
//   n_witness     = 1 + bits + 2 L + T + 3 S                        = 27 bits - 21 + T + 3 S
//   n_constraints = bits + 1 + L + 2 + L + 3 S + 1 + T              = 27 bits - 18 + 3 S + T
// (the rows in front of the cipher's are 27 bits - 19; the cipher adds its 3 S + 1 + T, tag row included), so n_witness - (n_constraints - 1) = -2.
// Both compilers allocate the public inputs first: epk, tag and ciphertext are known before the circuit runs (computed natively).  All elements canonical.
template <class FrP, int W>
static R1CS<FrP> hybrid_encrypt_circuit(bool witness_only, unsigned bits, const Fp<FrP>* init_canon, const Fp<FrP>* g_canon, const uint64_t* esk_words, const Fp<FrP>* pk_canon,
                                        const Fp<FrP>* epk_canon, const Fp<FrP>& tag_canon, const Fp<FrP>* ct_canon, const Fp<FrP>* header_canon, size_t header_len,
                                        const Fp<FrP>* text_canon, size_t blocks, const Fp<FrP>& a_canon, const Fp<FrP>& d_canon) {
    using F = Fp<FrP>;
    using V = FpVar<FrP>;
    static const poseidon::Constants<FrP, W> consts;
    const size_t n_text = blocks * (W - 1);
    R1CS<FrP> cs = witness_only ? R1CS<FrP>::for_witness() : R1CS<FrP>::for_proofs();
    const edwards::Coeffs<FrP> k{zl::to_mont(a_canon), zl::to_mont(d_canon)};
    const edwards::PointVar<FrP> g{cs.new_input(zl::to_mont(g_canon[0])), cs.new_input(zl::to_mont(g_canon[1]))};
    const edwards::PointVar<FrP> pk{cs.new_input(zl::to_mont(pk_canon[0])), cs.new_input(zl::to_mont(pk_canon[1]))};
    const V epk_x = cs.new_input(zl::to_mont(epk_canon[0])), epk_y = cs.new_input(zl::to_mont(epk_canon[1]));
    const V pub_tag = cs.new_input(zl::to_mont(tag_canon));
    std::vector<V> pub_ct(n_text), hv(header_len), pv(n_text), cv;
    for (size_t i = 0; i < n_text; i++) pub_ct[i] = cs.new_input(zl::to_mont(ct_canon[i]));
    for (size_t i = 0; i < header_len; i++) hv[i] = cs.new_input(zl::to_mont(header_canon[i]));
    F esk_canon;
    memcpy(esk_canon.l, esk_words, 32);
    const V esk = cs.new_witness(zl::to_mont(esk_canon));
    const std::vector<V> b = edwards::scalar_bits(esk, esk_words, bits, cs);
    const edwards::PointVar<FrP> epk = edwards::scalar_mul_le(k, g, b, cs);
    cs.enforce_equal(epk.x, epk_x);
    cs.enforce_equal(epk.y, epk_y);
    const edwards::PointVar<FrP> shared = edwards::scalar_mul_le(k, pk, b, cs);
    for (size_t i = 0; i < n_text; i++) pv[i] = cs.new_witness(zl::to_mont(text_canon[i]));
    V state[W];
    for (int i = 0; i < W; i++) state[i] = cs.constant(zl::to_mont(init_canon[i]));
    poseidon::duplex_encrypt_circuit<FrP, W>(consts, state, std::vector<V>{shared.x, shared.y}, hv, pv, cv, cs);
    cs.enforce_equal(state[1], pub_tag);
    for (size_t i = 0; i < n_text; i++) cs.enforce_equal(cv[i], pub_ct[i]);
    return cs;
}

}  // namespace openzl

// ------------------------------------------------------------------------------------------------ C-ABI hooks
// (struct zl_circuit and struct zl_g16_keys: zl_host_api.h)
using namespace openzl;
// include/zl_backend_test.h: turn the circuit into a DIFFERENT circuit of the same shape (first coefficient of A's row 0 doubled); its
// cached CSR export is dropped.  A proving context bound to the original circuit must refuse it (R1CS::structure_digest).
extern "C" int zl_test_circuit_tweak(zl_circuit* c) {
    if (!c) return ZL_EINVAL;
    if (c->bls) { c->bls->tweak_for_tests(); c->ex_bls = R1csExport<BLS12_381_Fr>(); c->ex_bls.build(*c->bls); }
    if (c->bn) { c->bn->tweak_for_tests(); c->ex_bn = R1csExport<BN254_Fr>(); c->ex_bn.build(*c->bn); }
    return ZL_OK;
}

template <class E> static const R1CS<typename E::FrP>* cs_of(const zl_circuit* c);
template <> const R1CS<BLS12_381_Fr>* cs_of<Bls12_381>(const zl_circuit* c) { return c->bls; }
template <> const R1CS<BN254_Fr>* cs_of<Bn254>(const zl_circuit* c) { return c->bn; }
// A stream of proofs over one key on two prover lanes (include/zl_backend.h): two host threads draw indices from one counter; thread 0 is the caller's
template <class E>
static int prove_circuits_t(zl_ctx* ctx, const typename Groth16<E>::ProvingContext& pc, const zl_circuit* const* circuits, const uint64_t* seeds, size_t count,
                            zl_g16_proof* proofs) {
    if (pc.ctx != ctx || ctx->parent || !pc.r1cs) return ZL_EINVAL;
    if (count > 1 && !ctx->stream_lane_ctx) {
        const int rc = zl_ctx_fork(ctx, &ctx->stream_lane_ctx);
        if (rc) return rc;
    }
    std::atomic<size_t> next{0};
    std::atomic<int> first_err{ZL_OK};
    auto work = [&](zl_ctx* lane) {
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= count || first_err.load() != ZL_OK) return;
            const zl_circuit* c = circuits[i];
            int rc = ZL_EINVAL;
            if (c && c->curve == E::curve) {
                SplitMix64 rng(seeds[i]);
                const auto* cs = cs_of<E>(c);
                auto res = Groth16<E>::prove(pc, *cs, rng, nullptr, nullptr, lane);
                rc = res.ok ? ZL_OK : res.error.code;
                if (res.ok) proofs[i] = res.value;
            }
            if (rc != ZL_OK) { int exp = ZL_OK; first_err.compare_exchange_strong(exp, rc); return; }
        }
    };
    if (count > 1) {
        std::thread second(work, ctx->stream_lane_ctx);
        work(ctx);
        second.join();
    } else {
        work(ctx);
    }
    return first_err.load();
}

// n canonical elements -> Fp words (still canonical); false when one is not below r
template <class FrP>
static bool elems_below_r(const uint64_t* w, size_t n, std::vector<Fp<FrP>>& out) {
    out.resize(n);
    for (size_t e = 0; e < n; e++) {
        memcpy(out[e].l, w + 4 * e, 32);
        bool lt = false;
        for (int i = FrP::N - 1; i >= 0; i--) {
            if (out[e].l[i] < FrP::mod(i)) { lt = true; break; }
            if (out[e].l[i] > FrP::mod(i)) break;
        }
        if (!lt) return false;
    }
    return true;
}
static void circuit_set(zl_circuit* c, R1CS<BLS12_381_Fr>&& cs) { c->bls = new R1CS<BLS12_381_Fr>(std::move(cs)); c->ex_bls.build(*c->bls); }
static void circuit_set(zl_circuit* c, R1CS<BN254_Fr>&& cs) { c->bn = new R1CS<BN254_Fr>(std::move(cs)); c->ex_bn.build(*c->bn); }
template <class FrP>
static int circuit_arity_t(zl_circuit* c, unsigned arity, const uint64_t* in, unsigned depth, uint64_t index, const uint64_t* path, bool witness_only) {
    std::vector<Fp<FrP>> x, pa;
    if (!elems_below_r<FrP>(in, arity, x) || !elems_below_r<FrP>(path, depth, pa)) return ZL_EINVAL;
    switch (arity) {
    case 2: circuit_set(c, poseidon_arity<FrP, 3>(witness_only, x.data(), depth, index, pa.data())); break;
    case 3: circuit_set(c, poseidon_arity<FrP, 4>(witness_only, x.data(), depth, index, pa.data())); break;
    case 4: circuit_set(c, poseidon_arity<FrP, 5>(witness_only, x.data(), depth, index, pa.data())); break;
    default: circuit_set(c, poseidon_arity<FrP, 6>(witness_only, x.data(), depth, index, pa.data())); break;
    }
    return ZL_OK;
}
// depth == 0: the hash circuit (no index, no path); otherwise the leaf-membership circuit
static int circuit_arity(zl_curve_t curve, unsigned arity, const uint64_t* in, unsigned depth, uint64_t index, const uint64_t* path, bool witness_only, zl_circuit** out) {
    if (!out || !in || arity < 2 || arity > 5 || (depth && !path) || depth > 40 || (index >> depth) || (curve != ZL_BLS12_381 && curve != ZL_BN254)) return ZL_EINVAL;
    zl_circuit* c = new (std::nothrow) zl_circuit();
    if (!c) return ZL_ENOMEM;
    c->curve = curve;
    const int rc = curve == ZL_BLS12_381 ? circuit_arity_t<BLS12_381_Fr>(c, arity, in, depth, index, path, witness_only)
                                         : circuit_arity_t<BN254_Fr>(c, arity, in, depth, index, path, witness_only);
    if (rc) {
        zl_circuit_free(c);
        return rc;
    }
    *out = c;
    return ZL_OK;
}
template <class FrP>
static int circuit_encrypt_t(zl_circuit* c, unsigned width, const uint64_t* initial_state, const uint64_t* key, size_t key_len, const uint64_t* header, size_t header_len,
                             const uint64_t* plaintext, size_t blocks, bool witness_only) {
    std::vector<Fp<FrP>> st, k, h, p;
    const uint64_t zero_state[4 * 6] = {0};
    if (!elems_below_r<FrP>(initial_state ? initial_state : zero_state, width, st) || !elems_below_r<FrP>(key, key_len, k) ||
        !elems_below_r<FrP>(header, header_len, h) || !elems_below_r<FrP>(plaintext, blocks * (width - 1), p))
        return ZL_EINVAL;
    switch (width) {
    case 3: circuit_set(c, poseidon_encrypt<FrP, 3>(witness_only, st.data(), k.data(), key_len, h.data(), header_len, p.data(), blocks)); break;
    case 4: circuit_set(c, poseidon_encrypt<FrP, 4>(witness_only, st.data(), k.data(), key_len, h.data(), header_len, p.data(), blocks)); break;
    case 5: circuit_set(c, poseidon_encrypt<FrP, 5>(witness_only, st.data(), k.data(), key_len, h.data(), header_len, p.data(), blocks)); break;
    default: circuit_set(c, poseidon_encrypt<FrP, 6>(witness_only, st.data(), k.data(), key_len, h.data(), header_len, p.data(), blocks)); break;
    }
    return ZL_OK;
}
static int circuit_encrypt(zl_curve_t curve, unsigned width, const uint64_t* initial_state, const uint64_t* key, size_t key_len, const uint64_t* header, size_t header_len,
                           const uint64_t* plaintext, size_t blocks, bool witness_only, zl_circuit** out) {
    if (!out || !key || key_len < 1 || (header_len && !header) || !plaintext || (curve != ZL_BLS12_381 && curve != ZL_BN254) ||
        zl_poseidon_duplex_permutations(width, key_len, header_len, blocks) == 0)
        return ZL_EINVAL;
    zl_circuit* c = new (std::nothrow) zl_circuit();
    if (!c) return ZL_ENOMEM;
    c->curve = curve;
    const int rc = curve == ZL_BLS12_381 ? circuit_encrypt_t<BLS12_381_Fr>(c, width, initial_state, key, key_len, header, header_len, plaintext, blocks, witness_only)
                                         : circuit_encrypt_t<BN254_Fr>(c, width, initial_state, key, key_len, header, header_len, plaintext, blocks, witness_only);
    if (rc) {
        zl_circuit_free(c);
        return rc;
    }
    *out = c;
    return ZL_OK;
}

template <class FrP>
static int circuit_ed_mul_t(zl_circuit* c, unsigned bits, const uint64_t* point_xy, const uint64_t* scalar, const uint64_t* q_xy, const uint64_t* a, const uint64_t* d,
                            bool witness_only) {
    std::vector<Fp<FrP>> p, q, ka, kd;
    if (!elems_below_r<FrP>(point_xy, 2, p) || !elems_below_r<FrP>(q_xy, 2, q) || !elems_below_r<FrP>(a, 1, ka) || !elems_below_r<FrP>(d, 1, kd)) return ZL_EINVAL;
    circuit_set(c, ed_scalar_mul_circuit<FrP>(witness_only, bits, p.data(), scalar, q.data(), ka[0], kd[0]));
    return ZL_OK;
}
// Q = s P natively first (zl_ed_scalar_mul: it refuses a coordinate >= q, a point off the curve and a scalar >= l), then the circuit around it
static int circuit_ed_mul(zl_curve_t curve, unsigned bits, const uint64_t* point_xy, const uint64_t* scalar, bool witness_only, zl_circuit** out) {
    if (!out || !point_xy || !scalar || zl_ed_scalar_mul_assignment_elems(curve, bits) == 0) return ZL_EINVAL;
    for (unsigned i = bits; i < 256; i++)
        if ((scalar[i >> 6] >> (i & 63)) & 1) return ZL_EINVAL;  // s >= 2^bits
    uint64_t q[8], a[4], d[4];
    if (zl_ed_scalar_mul(curve, point_xy, scalar, q) || zl_ed_params(curve, a, d, nullptr, nullptr)) return ZL_EINVAL;
    zl_circuit* c = new (std::nothrow) zl_circuit();
    if (!c) return ZL_ENOMEM;
    c->curve = curve;
    const int rc = curve == ZL_BLS12_381 ? circuit_ed_mul_t<BLS12_381_Fr>(c, bits, point_xy, scalar, q, a, d, witness_only)
                                         : circuit_ed_mul_t<BN254_Fr>(c, bits, point_xy, scalar, q, a, d, witness_only);
    if (rc) {
        zl_circuit_free(c);
        return rc;
    }
    *out = c;
    return ZL_OK;
}

struct HybridCircuitIn {
    unsigned width, bits;
    const uint64_t *initial_state, *generator_xy, *esk, *pk_xy, *header, *plaintext;
    size_t header_len, blocks;
    bool witness_only;
};
template <class FrP>
static int circuit_hybrid_t(zl_circuit* c, const HybridCircuitIn& in, const uint64_t* epk, const uint64_t* tag, const uint64_t* ct, const uint64_t* a, const uint64_t* d) {
    std::vector<Fp<FrP>> st, g, pk, e, tg, cv, h, p, ka, kd;
    const uint64_t zero_state[4 * 6] = {0};
    const size_t n_text = in.blocks * (in.width - 1);
    if (!elems_below_r<FrP>(in.initial_state ? in.initial_state : zero_state, in.width, st) || !elems_below_r<FrP>(in.generator_xy, 2, g) ||
        !elems_below_r<FrP>(in.pk_xy, 2, pk) || !elems_below_r<FrP>(epk, 2, e) || !elems_below_r<FrP>(tag, 1, tg) || !elems_below_r<FrP>(ct, n_text, cv) ||
        !elems_below_r<FrP>(in.header, in.header_len, h) || !elems_below_r<FrP>(in.plaintext, n_text, p) || !elems_below_r<FrP>(a, 1, ka) || !elems_below_r<FrP>(d, 1, kd))
        return ZL_EINVAL;
#define ZL_HYBRID_W(W)                                                                                                                                                  \
    circuit_set(c, hybrid_encrypt_circuit<FrP, W>(in.witness_only, in.bits, st.data(), g.data(), in.esk, pk.data(), e.data(), tg[0], cv.data(), h.data(), in.header_len, \
                                                  p.data(), in.blocks, ka[0], kd[0]))
    switch (in.width) {
    case 3: ZL_HYBRID_W(3); break;
    case 4: ZL_HYBRID_W(4); break;
    case 5: ZL_HYBRID_W(5); break;
    default: ZL_HYBRID_W(6); break;
    }
#undef ZL_HYBRID_W
    return ZL_OK;
}
// epk, tag and ciphertext natively first (zl_hybrid_encrypt_batch's host mirror: it refuses a coordinate >= q, a point off the curve, esk >= l and an element
// >= r), then the circuit around them
static int circuit_hybrid(zl_curve_t curve, const HybridCircuitIn& in, zl_circuit** out) {
    if (!out || !in.generator_xy || !in.esk || !in.pk_xy || (in.header_len && !in.header) || !in.plaintext ||
        zl_hybrid_encrypt_assignment_elems(curve, in.width, in.bits, in.header_len, in.blocks) == 0)
        return ZL_EINVAL;
    for (unsigned i = in.bits; i < 256; i++)
        if ((in.esk[i >> 6] >> (i & 63)) & 1) return ZL_EINVAL;  // esk >= 2^bits
    uint64_t epk[8], tag[4], a[4], d[4];
    std::vector<uint64_t> ct(in.blocks * (in.width - 1) * 4);
    if (zl_hybrid_encrypt_batch(nullptr, curve, in.width, in.initial_state, in.generator_xy, in.esk, in.pk_xy, 1, in.header, in.header_len, in.plaintext, in.blocks, 1, 0, epk,
                                ct.data(), tag, nullptr) ||
        zl_ed_params(curve, a, d, nullptr, nullptr))
        return ZL_EINVAL;
    zl_circuit* c = new (std::nothrow) zl_circuit();
    if (!c) return ZL_ENOMEM;
    c->curve = curve;
    const int rc = curve == ZL_BLS12_381 ? circuit_hybrid_t<BLS12_381_Fr>(c, in, epk, tag, ct.data(), a, d) : circuit_hybrid_t<BN254_Fr>(c, in, epk, tag, ct.data(), a, d);
    if (rc) {
        zl_circuit_free(c);
        return rc;
    }
    *out = c;
    return ZL_OK;
}

extern "C" {

int zl_circuit_hybrid_encrypt(zl_curve_t curve, unsigned width, unsigned bits, const uint64_t* initial_state, const uint64_t* generator_xy, const uint64_t* esk,
                              const uint64_t* pk_xy, const uint64_t* header, size_t header_len, const uint64_t* plaintext, size_t blocks, zl_circuit** out) {
    return circuit_hybrid(curve, HybridCircuitIn{width, bits, initial_state, generator_xy, esk, pk_xy, header, plaintext, header_len, blocks, false}, out);
}
int zl_circuit_hybrid_encrypt_witness(zl_curve_t curve, unsigned width, unsigned bits, const uint64_t* initial_state, const uint64_t* generator_xy, const uint64_t* esk,
                                      const uint64_t* pk_xy, const uint64_t* header, size_t header_len, const uint64_t* plaintext, size_t blocks, zl_circuit** out) {
    return circuit_hybrid(curve, HybridCircuitIn{width, bits, initial_state, generator_xy, esk, pk_xy, header, plaintext, header_len, blocks, true}, out);
}
int zl_circuit_ed_scalar_mul(zl_curve_t curve, unsigned bits, const uint64_t* point_xy, const uint64_t* scalar, zl_circuit** out) {
    return circuit_ed_mul(curve, bits, point_xy, scalar, false, out);
}
int zl_circuit_ed_scalar_mul_witness(zl_curve_t curve, unsigned bits, const uint64_t* point_xy, const uint64_t* scalar, zl_circuit** out) {
    return circuit_ed_mul(curve, bits, point_xy, scalar, true, out);
}
int zl_circuit_witness_only_compatible(const zl_circuit* c) {
    if (!c) return ZL_EINVAL;
    return c->curve == ZL_BLS12_381 ? (c->bls->witness_only_compatible() ? 1 : 0) : (c->bn->witness_only_compatible() ? 1 : 0);
}
int zl_circuit_poseidon_encrypt(zl_curve_t curve, unsigned width, const uint64_t* initial_state, const uint64_t* key, size_t key_len, const uint64_t* header,
                                size_t header_len, const uint64_t* plaintext, size_t blocks, zl_circuit** out) {
    return circuit_encrypt(curve, width, initial_state, key, key_len, header, header_len, plaintext, blocks, false, out);
}
int zl_circuit_poseidon_encrypt_witness(zl_curve_t curve, unsigned width, const uint64_t* initial_state, const uint64_t* key, size_t key_len, const uint64_t* header,
                                        size_t header_len, const uint64_t* plaintext, size_t blocks, zl_circuit** out) {
    return circuit_encrypt(curve, width, initial_state, key, key_len, header, header_len, plaintext, blocks, true, out);
}
int zl_circuit_poseidon_chain(zl_curve_t curve, uint32_t k, const uint64_t* x0, const uint64_t* x1, zl_circuit** out) {
    if (!out || !x0 || !x1 || k == 0 || (curve != ZL_BLS12_381 && curve != ZL_BN254)) return ZL_EINVAL;
    zl_circuit* c = new (std::nothrow) zl_circuit();
    if (!c) return ZL_ENOMEM;
    c->curve = curve;
    if (curve == ZL_BLS12_381) {
        Fp<BLS12_381_Fr> a, b;
        memcpy(a.l, x0, 32); memcpy(b.l, x1, 32);
        const auto t0 = std::chrono::steady_clock::now();
        c->bls = new R1CS<BLS12_381_Fr>(poseidon_chain<BLS12_381_Fr>(k, a, b));
        const auto t1 = std::chrono::steady_clock::now();
        c->ex_bls.build(*c->bls);
        if (getenv("ZL_DEBUG_TIMING"))
            fprintf(stderr, "[zl] poseidon_chain %.3f s, export %.3f s\n", std::chrono::duration<double>(t1 - t0).count(),
                    std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count());
    } else {
        Fp<BN254_Fr> a, b;
        memcpy(a.l, x0, 32); memcpy(b.l, x1, 32);
        c->bn = new R1CS<BN254_Fr>(poseidon_chain<BN254_Fr>(k, a, b));
        c->ex_bn.build(*c->bn);
    }
    *out = c;
    return ZL_OK;
}
// the same circuit synthesised by a witness-only compiler (values, no rows): for proofs against a context that already holds the circuit's matrices
int zl_circuit_poseidon_chain_witness(zl_curve_t curve, uint32_t k, const uint64_t* x0, const uint64_t* x1, zl_circuit** out) {
    if (!out || !x0 || !x1 || k == 0 || (curve != ZL_BLS12_381 && curve != ZL_BN254)) return ZL_EINVAL;
    zl_circuit* c = new (std::nothrow) zl_circuit();
    if (!c) return ZL_ENOMEM;
    c->curve = curve;
    if (curve == ZL_BLS12_381) {
        Fp<BLS12_381_Fr> a, b;
        memcpy(a.l, x0, 32); memcpy(b.l, x1, 32);
        c->bls = new R1CS<BLS12_381_Fr>(poseidon_chain_witness<BLS12_381_Fr>(k, a, b));
        c->ex_bls.build(*c->bls);  // (no rows: only the assignment is exported)
    } else {
        Fp<BN254_Fr> a, b;
        memcpy(a.l, x0, 32); memcpy(b.l, x1, 32);
        c->bn = new R1CS<BN254_Fr>(poseidon_chain_witness<BN254_Fr>(k, a, b));
        c->ex_bn.build(*c->bn);
    }
    *out = c;
    return ZL_OK;
}
static int circuit_merkle(zl_curve_t curve, unsigned depth, const uint64_t* leaf, uint64_t index, const uint64_t* path, bool witness_only, zl_circuit** out) {
    if (!out || !leaf || !path || depth < 1 || depth > 40 || (index >> depth) || (curve != ZL_BLS12_381 && curve != ZL_BN254)) return ZL_EINVAL;
    zl_circuit* c = new (std::nothrow) zl_circuit();
    if (!c) return ZL_ENOMEM;
    c->curve = curve;
    if (curve == ZL_BLS12_381) {
        Fp<BLS12_381_Fr> lf;
        std::vector<Fp<BLS12_381_Fr>> pa(depth);
        memcpy(lf.l, leaf, 32);
        for (unsigned j = 0; j < depth; j++) memcpy(pa[j].l, path + 4 * j, 32);
        c->bls = new R1CS<BLS12_381_Fr>(witness_only ? poseidon_merkle_witness<BLS12_381_Fr>(depth, lf, index, pa.data())
                                                     : poseidon_merkle<BLS12_381_Fr>(depth, lf, index, pa.data()));
        c->ex_bls.build(*c->bls);
    } else {
        Fp<BN254_Fr> lf;
        std::vector<Fp<BN254_Fr>> pa(depth);
        memcpy(lf.l, leaf, 32);
        for (unsigned j = 0; j < depth; j++) memcpy(pa[j].l, path + 4 * j, 32);
        c->bn = new R1CS<BN254_Fr>(witness_only ? poseidon_merkle_witness<BN254_Fr>(depth, lf, index, pa.data())
                                                : poseidon_merkle<BN254_Fr>(depth, lf, index, pa.data()));
        c->ex_bn.build(*c->bn);
    }
    *out = c;
    return ZL_OK;
}
int zl_circuit_poseidon_merkle(zl_curve_t curve, unsigned depth, const uint64_t* leaf, uint64_t index, const uint64_t* path, zl_circuit** out) {
    return circuit_merkle(curve, depth, leaf, index, path, false, out);
}
int zl_circuit_poseidon_merkle_witness(zl_curve_t curve, unsigned depth, const uint64_t* leaf, uint64_t index, const uint64_t* path, zl_circuit** out) {
    return circuit_merkle(curve, depth, leaf, index, path, true, out);
}
int zl_circuit_poseidon_hash(zl_curve_t curve, unsigned arity, const uint64_t* in, zl_circuit** out) {
    return circuit_arity(curve, arity, in, 0, 0, nullptr, false, out);
}
int zl_circuit_poseidon_hash_witness(zl_curve_t curve, unsigned arity, const uint64_t* in, zl_circuit** out) {
    return circuit_arity(curve, arity, in, 0, 0, nullptr, true, out);
}
int zl_circuit_poseidon_merkle_leaf(zl_curve_t curve, unsigned arity, unsigned depth, const uint64_t* preimage, uint64_t index, const uint64_t* path, zl_circuit** out) {
    if (depth < 1) return ZL_EINVAL;
    return circuit_arity(curve, arity, preimage, depth, index, path, false, out);
}
int zl_circuit_poseidon_merkle_leaf_witness(zl_curve_t curve, unsigned arity, unsigned depth, const uint64_t* preimage, uint64_t index, const uint64_t* path,
                                            zl_circuit** out) {
    if (depth < 1) return ZL_EINVAL;
    return circuit_arity(curve, arity, preimage, depth, index, path, true, out);
}
void zl_circuit_free(zl_circuit* c) {
    if (!c) return;
    delete c->bls;
    delete c->bn;
    delete c;
}
int zl_circuit_export(const zl_circuit* c, zl_r1cs* view, const uint64_t** assignment) {
    if (!c || !view) return ZL_EINVAL;
    if (c->curve == ZL_BLS12_381) { *view = c->ex_bls.view; if (assignment) *assignment = c->ex_bls.assignment.data(); }
    else { *view = c->ex_bn.view; if (assignment) *assignment = c->ex_bn.assignment.data(); }
    return ZL_OK;
}
int zl_circuit_is_satisfied(const zl_circuit* c) {
    if (!c) return ZL_EINVAL;
    return c->curve == ZL_BLS12_381 ? (c->bls->is_satisfied() ? 1 : 0) : (c->bn->is_satisfied() ? 1 : 0);
}
int zl_poseidon_permute(zl_curve_t curve, uint64_t* state) {
    if (!state) return ZL_EINVAL;
    if (curve == ZL_BLS12_381) {
        static const poseidon::Constants<BLS12_381_Fr> cst;
        Fp<BLS12_381_Fr> st[3];
        for (int i = 0; i < 3; i++) { memcpy(st[i].l, state + 4 * i, 32); st[i] = zl::to_mont(st[i]); }
        poseidon::permute_native(cst, st);
        for (int i = 0; i < 3; i++) { st[i] = zl::from_mont(st[i]); memcpy(state + 4 * i, st[i].l, 32); }
        return ZL_OK;
    }
    if (curve == ZL_BN254) {
        static const poseidon::Constants<BN254_Fr> cst;
        Fp<BN254_Fr> st[3];
        for (int i = 0; i < 3; i++) { memcpy(st[i].l, state + 4 * i, 32); st[i] = zl::to_mont(st[i]); }
        poseidon::permute_native(cst, st);
        for (int i = 0; i < 3; i++) { st[i] = zl::from_mont(st[i]); memcpy(state + 4 * i, st[i].l, 32); }
        return ZL_OK;
    }
    return ZL_EINVAL;
}
int zl_groth16_compile(zl_ctx* ctx, const zl_circuit* c, uint64_t seed, zl_g16_keys** out) {
    if (!ctx || !c || !out) return ZL_EINVAL;
    zl_g16_keys* k = new (std::nothrow) zl_g16_keys();
    if (!k) return ZL_ENOMEM;
    k->curve = c->curve;
    SplitMix64 rng(seed);
    int rc = ZL_OK;
    if (c->curve == ZL_BLS12_381) {
        auto r = Groth16<Bls12_381>::compile(ctx, *c->bls, rng, &c->ex_bls);
        if (!r.ok) rc = r.error.code; else {
            k->pc_bls = r.value.first;
            k->vk_bls = r.value.second;
            for (auto& g : r.value.second.gamma_abc_exponents) { uint64_t w[4]; to_canon_words<BLS12_381_Fr>(w, g); k->gamma_abc.insert(k->gamma_abc.end(), w, w + 4); }
        }
    } else {
        auto r = Groth16<Bn254>::compile(ctx, *c->bn, rng, &c->ex_bn);
        if (!r.ok) rc = r.error.code; else {
            k->pc_bn = r.value.first;
            k->vk_bn = r.value.second;
            for (auto& g : r.value.second.gamma_abc_exponents) { uint64_t w[4]; to_canon_words<BN254_Fr>(w, g); k->gamma_abc.insert(k->gamma_abc.end(), w, w + 4); }
        }
    }
    if (rc) { delete k; return rc; }
    *out = k;
    return ZL_OK;
}
void zl_groth16_keys_free(zl_g16_keys* k) {
    if (!k) return;
    Groth16<Bls12_381>::release(k->pc_bls);
    Groth16<Bn254>::release(k->pc_bn);
    delete k;
}
int zl_groth16_keys_pk(const zl_g16_keys* k, zl_g16_pk* pk) {
    if (!k || !pk) return ZL_EINVAL;
    pk->curve = k->curve;
#define FILL(pc)                                                                                                     \
    pk->a_query = pc.a_query; pk->b_g1_query = pc.b_g1_query; pk->h_query = pc.h_query; pk->l_query = pc.l_query;    \
    pk->b_g2_query = pc.b_g2_query; pk->alpha_g1 = pc.alpha_g1.data(); pk->beta_g1 = pc.beta_g1.data();              \
    pk->delta_g1 = pc.delta_g1.data(); pk->beta_g2 = pc.beta_g2.data(); pk->delta_g2 = pc.delta_g2.data();
    if (k->curve == ZL_BLS12_381) { FILL(k->pc_bls) } else { FILL(k->pc_bn) }
#undef FILL
    return ZL_OK;
}
int zl_groth16_keys_trapdoor(const zl_g16_keys* k, uint64_t* out20) {
    if (!k || !out20) return ZL_EINVAL;
    if (!(k->curve == ZL_BLS12_381 ? k->pc_bls.has_trapdoor : k->pc_bn.has_trapdoor)) return ZL_EINVAL;  // keys decoded from bytes carry none
    if (k->curve == ZL_BLS12_381) {
        const auto& t = k->pc_bls.trapdoor;
        const Fp<BLS12_381_Fr>* v[5] = {&t.alpha, &t.beta, &t.gamma, &t.delta, &t.tau};
        for (int i = 0; i < 5; i++) memcpy(out20 + 4 * i, v[i]->l, 32);
    } else {
        const auto& t = k->pc_bn.trapdoor;
        const Fp<BN254_Fr>* v[5] = {&t.alpha, &t.beta, &t.gamma, &t.delta, &t.tau};
        for (int i = 0; i < 5; i++) memcpy(out20 + 4 * i, v[i]->l, 32);
    }
    return ZL_OK;
}
int zl_groth16_prove_circuit(zl_ctx* ctx, const zl_g16_keys* k, const zl_circuit* c, uint64_t seed, zl_g16_proof* proof, uint64_t* r_out, uint64_t* s_out) {
    if (!ctx || !k || !c || !proof || k->curve != c->curve) return ZL_EINVAL;
    SplitMix64 rng(seed);
    if (c->curve == ZL_BLS12_381) {
        Fp<BLS12_381_Fr> r, s;
        auto res = Groth16<Bls12_381>::prove(k->pc_bls, *c->bls, rng, &r, &s, ctx);
        if (!res.ok) return res.error.code;
        *proof = res.value;
        if (r_out) memcpy(r_out, r.l, 32);
        if (s_out) memcpy(s_out, s.l, 32);
    } else {
        Fp<BN254_Fr> r, s;
        auto res = Groth16<Bn254>::prove(k->pc_bn, *c->bn, rng, &r, &s, ctx);
        if (!res.ok) return res.error.code;
        *proof = res.value;
        if (r_out) memcpy(r_out, r.l, 32);
        if (s_out) memcpy(s_out, s.l, 32);
    }
    return ZL_OK;
}

int zl_groth16_prove_circuits(zl_ctx* ctx, const zl_g16_keys* k, const zl_circuit* const* circuits, const uint64_t* seeds, size_t count, zl_g16_proof* proofs) {
    if (!ctx || !k || (count && (!circuits || !seeds || !proofs))) return ZL_EINVAL;
    if (k->curve == ZL_BLS12_381) return prove_circuits_t<Bls12_381>(ctx, k->pc_bls, circuits, seeds, count, proofs);
    return prove_circuits_t<Bn254>(ctx, k->pc_bn, circuits, seeds, count, proofs);
}

// ---- ProvingContext / VerifyingKey wire formats (Groth16<E>::encode / decode / encode_verifying_key) ------------------------------
int zl_groth16_keys_to_bytes(const zl_g16_keys* k, uint8_t* out, size_t cap, size_t* len) {
    if (!k || !len || (!out && cap)) return ZL_EINVAL;
    Result<std::vector<uint8_t>> r = k->curve == ZL_BLS12_381 ? Groth16<Bls12_381>::encode(k->pc_bls, k->vk_bls) : Groth16<Bn254>::encode(k->pc_bn, k->vk_bn);
    if (!r.ok) return r.error.code;
    *len = r.value.size();
    if (cap < r.value.size()) return out ? ZL_EINVAL : ZL_OK;  // out == NULL, cap == 0: size query
    memcpy(out, r.value.data(), r.value.size());
    return ZL_OK;
}
int zl_groth16_keys_from_bytes(zl_ctx* ctx, zl_curve_t curve, const uint8_t* in, size_t len, unsigned flags, zl_g16_keys** out) {
    if (!ctx || !in || !out || (curve != ZL_BLS12_381 && curve != ZL_BN254) || (flags & ~ZL_CHECK)) return ZL_EINVAL;
    zl_g16_keys* k = new (std::nothrow) zl_g16_keys();
    if (!k) return ZL_ENOMEM;
    k->curve = curve;
    int rc = ZL_OK;
    if (curve == ZL_BLS12_381) {
        auto r = Groth16<Bls12_381>::decode(ctx, in, len, flags);
        if (!r.ok) rc = r.error.code; else { k->pc_bls = r.value.first; k->vk_bls = r.value.second; }
    } else {
        auto r = Groth16<Bn254>::decode(ctx, in, len, flags);
        if (!r.ok) rc = r.error.code; else { k->pc_bn = r.value.first; k->vk_bn = r.value.second; }
    }
    if (rc) { delete k; return rc; }
    *out = k;
    return ZL_OK;
}
// host-only validation of the same bytes (no ctx, no device): framing, lengths, canonical coordinates, flags; with ZL_CHECK the verifying-key points are also
// checked for curve / subgroup membership (the queries' curve checks happen on the device at upload).  What a service runs on untrusted input before it
// spends device memory on it, and the fuzz target of the sanitizer build (tests/test_sanitizers.py).
int zl_groth16_keys_parse(zl_curve_t curve, const uint8_t* in, size_t len, unsigned flags) {
    if (!in || (curve != ZL_BLS12_381 && curve != ZL_BN254) || (flags & ~ZL_CHECK)) return ZL_EINVAL;
    if (curve == ZL_BLS12_381) {
        auto r = Groth16<Bls12_381>::decode(nullptr, in, len, flags);
        return r.ok ? ZL_OK : r.error.code;
    }
    auto r = Groth16<Bn254>::decode(nullptr, in, len, flags);
    return r.ok ? ZL_OK : r.error.code;
}
int zl_groth16_vk_to_bytes(const zl_g16_keys* k, uint8_t* out, size_t cap, size_t* len) {
    if (!k || !len || (!out && cap)) return ZL_EINVAL;
    const std::vector<uint8_t> v = k->curve == ZL_BLS12_381 ? Groth16<Bls12_381>::encode_verifying_key(k->vk_bls) : Groth16<Bn254>::encode_verifying_key(k->vk_bn);
    *len = v.size();
    if (cap < v.size()) return out ? ZL_EINVAL : ZL_OK;
    memcpy(out, v.data(), v.size());
    return ZL_OK;
}
size_t zl_point_bytes_uncompressed(zl_curve_t curve, zl_group_t group) { return 2 * zl_point_bytes(curve, group); }
int zl_point_to_bytes_uncompressed(zl_curve_t curve, zl_group_t group, const uint64_t* xy, uint8_t inf, uint8_t* out) {
    if (!xy || !out || !zl_point_bytes(curve, group)) return ZL_EINVAL;
    if (curve == ZL_BLS12_381) { if (group == ZL_G1) serialize::BlsCodec::g1_to_uncompressed(xy, inf != 0, out); else serialize::BlsCodec::g2_to_uncompressed(xy, inf != 0, out); }
    else { if (group == ZL_G1) serialize::BnCodec::g1_to_uncompressed(xy, inf != 0, out); else serialize::BnCodec::g2_to_uncompressed(xy, inf != 0, out); }
    return ZL_OK;
}
int zl_point_from_bytes_uncompressed(zl_curve_t curve, zl_group_t group, const uint8_t* in, int check, uint64_t* xy, uint8_t* inf) {
    if (!xy || !in || !inf || !zl_point_bytes(curve, group)) return ZL_EINVAL;
    if (curve == ZL_BLS12_381) return group == ZL_G1 ? serialize::BlsCodec::g1_from_uncompressed(in, check != 0, xy, inf) : serialize::BlsCodec::g2_from_uncompressed(in, check != 0, xy, inf);
    return group == ZL_G1 ? serialize::BnCodec::g1_from_uncompressed(in, check != 0, xy, inf) : serialize::BnCodec::g2_from_uncompressed(in, check != 0, xy, inf);
}

// ---- wire proofs and points decoded on the device (zl_decode_dev.hip) ---------------------------------------------------------------------------------
int zl_points_from_bytes_batch(zl_ctx* ctx, zl_curve_t curve, zl_group_t group, const uint8_t* in, size_t count, uint64_t* out_xy, uint8_t* out_inf,
                               int32_t* status) {
    if (!ctx || !zl_point_bytes(curve, group)) return ZL_EINVAL;
    return curve == ZL_BLS12_381 ? decode_dev::points_bls(ctx, group, in, count, out_xy, out_inf, status) : decode_dev::points_bn(ctx, group, in, count, out_xy, out_inf, status);
}
int zl_groth16_proofs_from_bytes_batch(zl_ctx* ctx, zl_curve_t curve, const uint8_t* in, size_t count, zl_g16_proof* proofs, int32_t* status) {
    if (!ctx || !zl_groth16_proof_bytes(curve)) return ZL_EINVAL;
    return curve == ZL_BLS12_381 ? decode_dev::proofs_bls(ctx, in, count, proofs, status) : decode_dev::proofs_bn(ctx, in, count, proofs, status);
}
// ---- wire formats (arkworks CanonicalSerialize, compressed; zl_serialize.h) -----------------------------------------------------
size_t zl_point_bytes(zl_curve_t curve, zl_group_t group) {
    if ((curve != ZL_BLS12_381 && curve != ZL_BN254) || (group != ZL_G1 && group != ZL_G2)) return 0;
    const size_t nb = curve == ZL_BLS12_381 ? 48 : 32;
    return group == ZL_G1 ? nb : 2 * nb;
}
int zl_point_to_bytes(zl_curve_t curve, zl_group_t group, const uint64_t* xy, uint8_t inf, uint8_t* out) {
    if (!xy || !out || !zl_point_bytes(curve, group)) return ZL_EINVAL;
    if (curve == ZL_BLS12_381) { if (group == ZL_G1) serialize::BlsCodec::g1_to_bytes(xy, inf != 0, out); else serialize::BlsCodec::g2_to_bytes(xy, inf != 0, out); }
    else { if (group == ZL_G1) serialize::BnCodec::g1_to_bytes(xy, inf != 0, out); else serialize::BnCodec::g2_to_bytes(xy, inf != 0, out); }
    return ZL_OK;
}
int zl_point_from_bytes(zl_curve_t curve, zl_group_t group, const uint8_t* in, uint64_t* xy, uint8_t* inf) {
    if (!xy || !in || !inf || !zl_point_bytes(curve, group)) return ZL_EINVAL;
    if (curve == ZL_BLS12_381) return group == ZL_G1 ? serialize::BlsCodec::g1_from_bytes(in, xy, inf) : serialize::BlsCodec::g2_from_bytes(in, xy, inf);
    return group == ZL_G1 ? serialize::BnCodec::g1_from_bytes(in, xy, inf) : serialize::BnCodec::g2_from_bytes(in, xy, inf);
}
size_t zl_groth16_proof_bytes(zl_curve_t curve) { return 2 * zl_point_bytes(curve, ZL_G1) + zl_point_bytes(curve, ZL_G2); }
int zl_groth16_proof_to_bytes(zl_curve_t curve, const zl_g16_proof* proof, uint8_t* out) {
    if (!proof || !out || !zl_groth16_proof_bytes(curve)) return ZL_EINVAL;
    const size_t n1 = zl_point_bytes(curve, ZL_G1), n2 = zl_point_bytes(curve, ZL_G2);
    int rc;
    if ((rc = zl_point_to_bytes(curve, ZL_G1, proof->a, proof->a_inf, out))) return rc;
    if ((rc = zl_point_to_bytes(curve, ZL_G2, proof->b, proof->b_inf, out + n1))) return rc;
    return zl_point_to_bytes(curve, ZL_G1, proof->c, proof->c_inf, out + n1 + n2);
}
int zl_groth16_proof_from_bytes(zl_curve_t curve, const uint8_t* in, size_t len, zl_g16_proof* proof) {
    if (!proof || !in || !zl_groth16_proof_bytes(curve) || len != zl_groth16_proof_bytes(curve)) return ZL_EINVAL;
    const size_t n1 = zl_point_bytes(curve, ZL_G1), n2 = zl_point_bytes(curve, ZL_G2);
    memset(proof, 0, sizeof *proof);
    int rc;
    if ((rc = zl_point_from_bytes(curve, ZL_G1, in, proof->a, &proof->a_inf))) return rc;
    if ((rc = zl_point_from_bytes(curve, ZL_G2, in + n1, proof->b, &proof->b_inf))) return rc;
    return zl_point_from_bytes(curve, ZL_G1, in + n1 + n2, proof->c, &proof->c_inf);
}

}  // extern "C"
