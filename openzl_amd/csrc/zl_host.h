// zl_host.h -- host-side mirror (C++) of the reference's plugin interface for the Groth16 path, above the C ABI.
//
// The reference is Rust; this image has no Rust toolchain, so the operator/plugin surface that sits on top of the
// accelerated path is restated in C++ with the reference's names and argument meaning:
//   openzl::R1CS<F>            plugins/arkworks/src/constraint/mod.rs:64-108 (compiler wrapping a constraint system;
//                              for_contexts :84-90, for_proofs :94-99, Measure :147-177, allocation :210-338)
//   openzl::FpVar<F>           ark-r1cs-std FpVar as the plugin uses it: linear ops cost no constraint, mul costs one
//   openzl::poseidon::*        openzl-crypto/src/poseidon (lfsr.rs:14-100, round_constants.rs:10-59, mds.rs:84-102,
//                              mod.rs:193-282, hash.rs:93-135) + plugin Spec ops plugins/arkworks/src/poseidon/mod.rs:225-298
//   openzl::Groth16<E>         plugins/arkworks/src/groth16.rs:399-467: context_compiler / proof_compiler / compile /
//                              prove / verify with ProvingContext / VerifyingContext / Proof / Error
// Only what config 5 (Poseidon-hash circuit) needs is built; everything else of the gadget stack is out of scope.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <utility>
#include <vector>
#include <mutex>
#include "zl_ctx.h"
#include "zl_pairing.h"
#include "zl_poseidon_dev.h"  // poseidon_dev::spec: the (arity, width, rounds, tag) table

namespace openzl {

// ---- deterministic rng handed to compile / prove (the reference passes `&mut R: CryptoRng + RngCore`) ----------------
struct SplitMix64 {
    uint64_t s;
    explicit SplitMix64(uint64_t seed) : s(seed) {}
    uint64_t next() {
        s += 0x9E3779B97F4A7C15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
};
// uniform field element: fill limbs, mask to MODULUS_BITS, reject >= p (ark UniformRand for Fp; canonical here)
template <class FrP>
Fp<FrP> sample_canonical(SplitMix64& rng) {
    for (;;) {
        Fp<FrP> v;
        for (int i = 0; i < FrP::N; i += 2) {
            uint64_t w = rng.next();
            v.l[i] = (uint32_t)w;
            v.l[i + 1] = (uint32_t)(w >> 32);
        }
        const int top_bits = FrP::BITS - 32 * (FrP::N - 1);
        if (top_bits < 32) v.l[FrP::N - 1] &= (1u << top_bits) - 1;
        bool lt = false;
        for (int i = FrP::N - 1; i >= 0; i--) {
            if (v.l[i] < FrP::mod(i)) { lt = true; break; }
            if (v.l[i] > FrP::mod(i)) break;
        }
        if (lt) return v;
    }
}

// ---- linear combinations / variables ----------------------------------------------------------------------------------
// variable key: bit 31 = witness block, low bits = index inside the block; instance index 0 is the constant ONE
static constexpr uint32_t kWitnessBit = 0x80000000u;
static constexpr uint32_t kOne = 0;

template <class FrP>
struct LinearCombination {
    using F = Fp<FrP>;
    std::vector<std::pair<uint32_t, F>> terms;  // sorted by key, no zero coefficients
    static LinearCombination constant(const F& c) {
        LinearCombination r;
        if (!c.is_zero()) r.terms.push_back({kOne, c});
        return r;
    }
    static LinearCombination variable(uint32_t key) {
        LinearCombination r;
        r.terms.push_back({key, F::one()});
        return r;
    }
    bool is_constant() const { return terms.empty() || (terms.size() == 1 && terms[0].first == kOne); }
    LinearCombination add(const LinearCombination& o) const {
        LinearCombination r;
        r.terms.reserve(terms.size() + o.terms.size());
        size_t i = 0, j = 0;
        while (i < terms.size() || j < o.terms.size()) {
            if (j == o.terms.size() || (i < terms.size() && terms[i].first < o.terms[j].first)) r.terms.push_back(terms[i++]);
            else if (i == terms.size() || o.terms[j].first < terms[i].first) r.terms.push_back(o.terms[j++]);
            else {
                F s = zl::add(terms[i].second, o.terms[j].second);
                if (!s.is_zero()) r.terms.push_back({terms[i].first, s});
                i++;
                j++;
            }
        }
        return r;
    }
    LinearCombination scale(const F& c) const {
        LinearCombination r;
        if (c.is_zero()) return r;
        r.terms.reserve(terms.size());
        for (auto& t : terms) r.terms.push_back({t.first, zl::mul(t.second, c)});
        return r;
    }
};

template <class FrP>
struct FpVar {
    using F = Fp<FrP>;
    LinearCombination<FrP> lc;
    F value;  // Montgomery; meaningful in proof mode only
    bool konst = false;  // a constant (no variable in it): tracked beside lc because a witness-only compiler keeps no linear combinations
};

// ---- R1CS<F>: the plugin's compiler (constraint/mod.rs:64-108) -----------------------------------------------------------
template <class FrP>
class R1CS {
public:
    using F = Fp<FrP>;
    using LC = LinearCombination<FrP>;
    enum class Mode { Setup, Prove, ProveWitnessOnly };
    static R1CS for_contexts() { return R1CS(Mode::Setup); }  // SynthesisMode::Setup (constraint/mod.rs:84-90)
    static R1CS for_proofs() { return R1CS(Mode::Prove); }    // SynthesisMode::Prove (constraint/mod.rs:94-99)
    // ark-relations' SynthesisMode::Prove { construct_matrices: false }: the circuit code runs, variables are allocated with their values, but no linear
    // combination is formed and no constraint row stored.  What a prover needs per proof once its ProvingContext holds the circuit's matrices on the device
    // (they are static per circuit): Groth16::prove takes such a compiler for a BOUND context and ships its assignment.  (round 5: 958 465 constraints
    // synthesise in ~0.1 s this way against 1.1 s with the rows; the binding cannot be checked -- no rows to fingerprint -- so a witness-only compiler of another
    // circuit with the same variable counts yields a proof that does not verify, as a wrong witness would.)
    static R1CS for_witness() { return R1CS(Mode::ProveWitnessOnly); }
    bool witness_only() const { return mode_ == Mode::ProveWitnessOnly; }

    // allocation: Public -> instance variable (new_input), Secret -> witness (new_witness) (constraint/mod.rs:302-338)
    FpVar<FrP> new_input(const F& value_mont) {
        instance_.push_back(value_mont);
        if (witness_only()) return FpVar<FrP>{LC{}, value_mont, false};
        return FpVar<FrP>{LC::variable((uint32_t)instance_.size() - 1), value_mont, false};
    }
    FpVar<FrP> new_witness(const F& value_mont) {
        witness_.push_back(value_mont);
        if (witness_only()) return FpVar<FrP>{LC{}, value_mont, false};
        return FpVar<FrP>{LC::variable(kWitnessBit | ((uint32_t)witness_.size() - 1)), value_mont, false};
    }
    FpVar<FrP> constant(const F& c_mont) const { return FpVar<FrP>{witness_only() ? LC{} : LC::constant(c_mont), c_mont, true}; }
    // linear operations: no constraints (plugins/arkworks/src/poseidon/mod.rs:225-274)
    FpVar<FrP> add(const FpVar<FrP>& a, const FpVar<FrP>& b) const {
        if (witness_only()) return FpVar<FrP>{LC{}, zl::add(a.value, b.value), a.konst && b.konst};
        return FpVar<FrP>{a.lc.add(b.lc), zl::add(a.value, b.value), a.konst && b.konst};
    }
    FpVar<FrP> add_const(const FpVar<FrP>& a, const F& c) const {
        if (witness_only()) return FpVar<FrP>{LC{}, zl::add(a.value, c), a.konst};
        return FpVar<FrP>{a.lc.add(LC::constant(c)), zl::add(a.value, c), a.konst};
    }
    FpVar<FrP> mul_const(const FpVar<FrP>& a, const F& c) const {
        if (witness_only()) return FpVar<FrP>{LC{}, zl::mul(a.value, c), a.konst};
        return FpVar<FrP>{a.lc.scale(c), zl::mul(a.value, c), a.konst};
    }
    // multiplication: one constraint a * b = out with a fresh witness; constants fold
    FpVar<FrP> mul(const FpVar<FrP>& a, const FpVar<FrP>& b) {
        // Constant folding: the full compiler decides from the linear combination (no variable term left), the witness-only compiler -- it forms no
        // linear combinations -- from the `konst` flag the operations above propagate.  The two rules differ for a combination whose variable terms CANCEL
        // (x - x: constant for the full compiler, konst = false); a circuit that contains one would allocate witnesses differently in the two modes and a
        // witness-only assignment would not line up with the resident matrices.  The full compiler therefore records any disagreement, and a
        // proving context bound from such a compiler refuses witness-only compilers (Groth16::prove).
        if (!witness_only() && (a.lc.is_constant() != a.konst || b.lc.is_constant() != b.konst)) fold_rules_disagree_ = true;
        if (witness_only() ? a.konst : a.lc.is_constant()) return mul_const(b, a.value);
        if (witness_only() ? b.konst : b.lc.is_constant()) return mul_const(a, b.value);
        FpVar<FrP> out = new_witness(zl::mul(a.value, b.value));
        if (witness_only()) return out;
        A_.push_back(a.lc);
        B_.push_back(b.lc);
        C_.push_back(out.lc);
        return out;
    }
    void enforce_equal(const FpVar<FrP>& a, const FpVar<FrP>& b) {  // a * 1 = b
        if (witness_only()) { equal_ok_ = equal_ok_ && a.value == b.value; return; }
        A_.push_back(a.lc);
        B_.push_back(LC::constant(F::one()));
        C_.push_back(b.lc);
    }
    // Boolean witness (constraint/mod.rs:242-258): one witness of value 0 or 1 and the row (ONE - b) * b = 0, C empty.  ALWAYS allocates, in every mode, so that
    // a witness-only compiler lines up with the full one.
    FpVar<FrP> new_boolean_witness(bool bit) {
        FpVar<FrP> b = new_witness(bit ? F::one() : F::zero());
        if (witness_only()) return b;
        A_.push_back(LC::constant(F::one()).add(b.lc.scale(minus_one())));
        B_.push_back(b.lc);
        C_.push_back(LC{});
        return b;
    }
    // out = b ? t : f (the plugin's conditionally_select on FpVar, constraint/mod.rs:354-390): one fresh witness and the row b * (t - f) = out - f.  No
    // constant folding: it ALWAYS allocates, in every mode.  b must be Boolean (new_boolean_witness).
    FpVar<FrP> select(const FpVar<FrP>& b, const FpVar<FrP>& t, const FpVar<FrP>& f) {
        FpVar<FrP> out = new_witness(b.value.is_zero() ? f.value : t.value);
        if (witness_only()) return out;
        const LC neg_f = f.lc.scale(minus_one());
        A_.push_back(b.lc);
        B_.push_back(t.lc.add(neg_f));
        C_.push_back(out.lc.add(neg_f));
        return out;
    }
    // out = b / a for a divisor the circuit knows to be non-zero: one fresh witness whose VALUE the caller supplies (a field division made on the host) and
    // the row a * out = b.  No constant folding: it ALWAYS allocates, in every mode, like select and new_boolean_witness.
    FpVar<FrP> mul_equals(const FpVar<FrP>& a, const FpVar<FrP>& b, const F& out_value_mont) {
        FpVar<FrP> out = new_witness(out_value_mont);
        if (witness_only()) return out;
        A_.push_back(a.lc);
        B_.push_back(out.lc);
        C_.push_back(b.lc);
        return out;
    }
    static F minus_one() { return zl::sub(F::zero(), F::one()); }
    bool equalities_hold() const { return equal_ok_; }  // witness-only: every enforce_equal saw equal values
    // full compiler: every multiplication folded constants the way a witness-only run of the same circuit code will (see mul)
    bool witness_only_compatible() const { return !fold_rules_disagree_; }
    // Measure (openzl-crypto/src/constraint.rs:151-188; plugin impl constraint/mod.rs:169-177)
    size_t constraint_count() const { return A_.size(); }
    size_t public_variable_count() const { return instance_.size() - 1; }
    size_t secret_variable_count() const { return witness_.size(); }
    size_t num_instance_variables() const { return instance_.size(); }  // ark: includes the constant ONE
    Mode mode() const { return mode_; }

    F eval(const LC& lc) const {
        F acc = F::zero();
        for (auto& t : lc.terms) {
            const F& v = (t.first & kWitnessBit) ? witness_[t.first & ~kWitnessBit] : instance_[t.first];
            acc = zl::add(acc, zl::mul(t.second, v));
        }
        return acc;
    }
    bool is_satisfied() const {
        if (witness_only()) return equal_ok_;  // no rows: only the enforced equalities can be checked
        for (size_t i = 0; i < A_.size(); i++)
            if (zl::mul(eval(A_[i]), eval(B_[i])) != eval(C_[i])) return false;
        return true;
    }
    // Repeated sub-circuits (a hash chain, a Merkle path, ...): append `copies` copies of the constraint rows [r0, r1); in copy j = 1..copies
    // every witness index >= w_from is shifted by j * shift, all other variables (instance block, earlier witnesses) stay.  The caller
    // supplies the values of the copies' witnesses (copies * shift of them, in allocation order).  This is exactly what synthesising the
    // sub-circuit `copies` more times would append when it is wired the same way each time -- without redoing the symbolic
    // linear-combination arithmetic (tests/test_host_mirror.py compares the result with the sequential Python builder).
    void replicate_rows(size_t r0, size_t r1, size_t copies, uint32_t w_from, uint32_t shift, const std::vector<F>& new_witness_values);
    static LC shifted(const LC& lc, uint32_t w_from, uint32_t delta) {
        LC r = lc;
        for (auto& t : r.terms)
            if ((t.first & kWitnessBit) && (t.first & ~kWitnessBit) >= w_from) t.first += delta;  // order of the sorted keys is preserved
        return r;
    }
    uint32_t var_index(uint32_t key) const { return (key & kWitnessBit) ? (uint32_t)instance_.size() + (key & ~kWitnessBit) : key; }
    const std::vector<LC>& rows(int m) const { return m == 0 ? A_ : m == 1 ? B_ : C_; }
    // 64-bit fingerprint of the constraint MATRICES (not the assignment): row / variable counts and the keys + coefficients of EVERY
    // row of every matrix (a sampled digest would let a circuit that differs only in unsampled rows through; hashing the 958 465-row
    // Poseidon chain costs a few ms, once per compiler).  A proving context records it when it learns its circuit and refuses a compiler whose
    // fingerprint differs: two different circuits of the same shape must not silently share device matrices.  Rows are append-only, so
    // the value is cached per (row count, variable counts): prove() pays for it once per compiler.
    uint64_t structure_digest() const {
        static std::mutex digest_mu;  // one compiler may be proven from several lanes at once (Groth16::prove(..., lane)): the cache below is filled once, under this lock
        std::lock_guard<std::mutex> lk(digest_mu);
        if (digest_rows_ == A_.size() && digest_inst_ == instance_.size() && digest_wit_ == witness_.size()) return digest_;
        uint64_t h = 0xCBF29CE484222325ull;
        auto mix = [&h](uint64_t v) { h = (h ^ v) * 0x9E3779B97F4A7C15ull; h ^= h >> 29; };
        mix(A_.size()); mix(instance_.size()); mix(witness_.size());
        const size_t rows = A_.size();
        for (int m = 0; m < 3; m++) {
            const std::vector<LC>& M = this->rows(m);
            for (size_t i = 0; i < rows; i++) {
                mix(M[i].terms.size());
                for (const auto& t : M[i].terms) { mix(t.first); for (int k = 0; k < F::N; k += 2) mix((uint64_t)t.second.l[k] | ((uint64_t)t.second.l[k + 1] << 32)); }
            }
        }
        digest_ = h;
        digest_rows_ = A_.size(); digest_inst_ = instance_.size(); digest_wit_ = witness_.size();
        return h;
    }
    // TEST ONLY (zl_test_circuit_tweak): doubles the first coefficient of row 0 of A -- a different circuit of the same shape
    void tweak_for_tests() {
        if (!A_.empty() && !A_[0].terms.empty()) A_[0].terms[0].second = zl::add(A_[0].terms[0].second, A_[0].terms[0].second);
        digest_rows_ = (size_t)-1;
    }
    const std::vector<F>& instance_assignment() const { return instance_; }
    const std::vector<F>& witness_assignment() const { return witness_; }

private:
    explicit R1CS(Mode m) : mode_(m) { instance_.push_back(F::one()); }
    Mode mode_;
    bool equal_ok_ = true, fold_rules_disagree_ = false;
    std::vector<F> instance_, witness_;
    std::vector<LC> A_, B_, C_;
    mutable uint64_t digest_ = 0;
    mutable size_t digest_rows_ = (size_t)-1, digest_inst_ = 0, digest_wit_ = 0;
};

// ---- Poseidon (config 5) ------------------------------------------------------------------------------------------------------
namespace poseidon {
// 80-bit Grain LFSR in self-shrinking mode (openzl-crypto/src/poseidon/lfsr.rs:14-100)
class GrainLFSR {
public:
    GrainLFSR(unsigned modulus_bits, unsigned width, unsigned rf, unsigned rp) {
        for (auto& b : state_) b = false;
        head_ = 0;
        append(2, 1);
        append(4, 0);
        append(12, modulus_bits);
        append(12, width);
        append(10, rf);
        append(10, rp);
        append(30, (1u << 30) - 1);
        for (int i = 0; i < 160; i++) update();
    }
    bool next() {
        bool bit = update();
        while (!bit) {
            update();
            bit = update();
        }
        return update();
    }

private:
    bool state_[80];
    unsigned head_;
    void append(unsigned n, uint64_t bits) {
        for (int i = (int)n - 1; i >= 0; i--) set_next((bits >> i) & 1);
    }
    bool set_next(bool b) {
        state_[head_] = b;
        head_ = (head_ + 1) % 80;
        return b;
    }
    bool bit(unsigned i) const { return state_[(i + head_) % 80]; }
    bool update() { return set_next(bit(62) ^ bit(51) ^ bit(38) ^ bit(23) ^ bit(13) ^ bit(0)); }
};

// The constants of one width (3..6: poseidon_dev::spec, zl_poseidon_dev.h); Constants<FrP> is the width-3, arity-2 instance of the in-circuit hash.
template <class FrP, int W = 3>
struct Constants {
    using F = Fp<FrP>;
    static_assert(poseidon_dev::width_ok(W), "widths 3..6: arity 2..5");
    static constexpr poseidon_dev::Spec SPEC = poseidon_dev::spec_of_width(W);  // (plugins/arkworks/src/poseidon/mod.rs:300-322)
    static constexpr int WIDTH = W, FULL_ROUNDS = (int)SPEC.full_rounds, PARTIAL_ROUNDS = (int)SPEC.partial_rounds;
    std::vector<F> round_keys;  // WIDTH * (RF + RP), Montgomery
    F mds[WIDTH][WIDTH];
    Constants() {
        // generate_round_constants: MODULUS_BITS bits big-endian per candidate, rejection (round_constants.rs:10-59)
        GrainLFSR lfsr(FrP::BITS, WIDTH, FULL_ROUNDS, PARTIAL_ROUNDS);
        while ((int)round_keys.size() < WIDTH * (FULL_ROUNDS + PARTIAL_ROUNDS)) {
            F v = F::zero();
            for (int b = FrP::BITS - 1; b >= 0; b--)
                if (lfsr.next()) v.l[b >> 5] |= 1u << (b & 31);
            bool lt = false;
            for (int i = FrP::N - 1; i >= 0; i--) {
                if (v.l[i] < FrP::mod(i)) { lt = true; break; }
                if (v.l[i] > FrP::mod(i)) break;
            }
            if (lt) round_keys.push_back(zl::to_mont(v));
        }
        // generate_mds: M[i][j] = 1 / (i + (t + j)) (mds.rs:84-102)
        for (int i = 0; i < WIDTH; i++)
            for (int j = 0; j < WIDTH; j++) mds[i][j] = zl::inv(zl::from_u64<FrP>((uint64_t)(i + WIDTH + j)));
    }
};
// native permutation (openzl-tutorials/src/poseidon.rs:165-222 schedule; COM = ()), any width of the table
template <class FrP, int W>
void permute_native(const Constants<FrP, W>& c, Fp<FrP> state[W]) {
    using F = Fp<FrP>;
    const int half = c.FULL_ROUNDS / 2;
    for (int rnd = 0; rnd < c.FULL_ROUNDS + c.PARTIAL_ROUNDS; rnd++) {
        for (int i = 0; i < W; i++) state[i] = zl::add(state[i], c.round_keys[W * rnd + i]);
        const int lanes = (rnd < half || rnd >= half + c.PARTIAL_ROUNDS) ? W : 1;
        for (int i = 0; i < lanes; i++) {
            F x2 = zl::sqr(state[i]), x4 = zl::sqr(x2);
            state[i] = zl::mul(x4, state[i]);
        }
        F nx[W];
        for (int i = 0; i < W; i++) {
            F acc = zl::mul(c.mds[i][0], state[0]);
            for (int j = 1; j < W; j++) acc = zl::add(acc, zl::mul(c.mds[i][j], state[j]));
            nx[i] = acc;
        }
        for (int i = 0; i < W; i++) state[i] = nx[i];
    }
}
// the same permutation, recording what the in-circuit version allocates: x^2, x^4, x^5 of every S-box whose input is not a constant
// (lane 0 of the first round is: the capacity element 2^arity - 1 plus a round key), in allocation order -- round order, lane order within a round;
// 8 W + partial - 1 S-boxes at width W: 78, 86, 95, 103 at widths 3..6.  skip0: the lanes of round 0 that are NOT recorded, one bit per lane -- lane 0 alone for
// a hash; the duplex cipher's circuit (poseidon_encrypt, zl_host.hip) also folds the rate lanes of its first permutation that hold no key element, and
// records every S-box of its later permutations (skip0 = 0)
template <class FrP, int W>
void permute_native_record(const Constants<FrP, W>& c, Fp<FrP> state[W], std::vector<Fp<FrP>>& rec, unsigned skip0 = 1u) {
    using F = Fp<FrP>;
    const int half = c.FULL_ROUNDS / 2;
    for (int rnd = 0; rnd < c.FULL_ROUNDS + c.PARTIAL_ROUNDS; rnd++) {
        for (int i = 0; i < W; i++) state[i] = zl::add(state[i], c.round_keys[W * rnd + i]);
        const int lanes = (rnd < half || rnd >= half + c.PARTIAL_ROUNDS) ? W : 1;
        for (int i = 0; i < lanes; i++) {
            const F x2 = zl::sqr(state[i]), x4 = zl::sqr(x2);
            state[i] = zl::mul(x4, state[i]);
            if (rnd != 0 || !((skip0 >> i) & 1)) { rec.push_back(x2); rec.push_back(x4); rec.push_back(state[i]); }
        }
        F nx[W];
        for (int i = 0; i < W; i++) {
            F acc = zl::mul(c.mds[i][0], state[0]);
            for (int j = 1; j < W; j++) acc = zl::add(acc, zl::mul(c.mds[i][j], state[j]));
            nx[i] = acc;
        }
        for (int i = 0; i < W; i++) state[i] = nx[i];
    }
}
// the in-circuit permutation on W variables, in place: what hash runs on (tag, inputs) and the duplex cipher's circuit (poseidon_encrypt, zl_host.hip) on
// its running state.  S-boxes are allocated in round order, lane order within a round, each as x^2, x^4, x^5; one whose input is a constant folds
template <class FrP, int W>
void permute(const Constants<FrP, W>& c, FpVar<FrP> state[W], R1CS<FrP>& compiler) {
    using V = FpVar<FrP>;
    const int half = c.FULL_ROUNDS / 2;
    for (int rnd = 0; rnd < c.FULL_ROUNDS + c.PARTIAL_ROUNDS; rnd++) {
        for (int i = 0; i < W; i++) state[i] = compiler.add_const(state[i], c.round_keys[W * rnd + i]);
        const int lanes = (rnd < half || rnd >= half + c.PARTIAL_ROUNDS) ? W : 1;
        for (int i = 0; i < lanes; i++) {  // apply_sbox = x^5 (plugins/arkworks/src/poseidon/mod.rs:287-298)
            V x2 = compiler.mul(state[i], state[i]);
            V x4 = compiler.mul(x2, x2);
            state[i] = compiler.mul(x4, state[i]);
        }
        V nx[W];
        for (int i = 0; i < W; i++) {
            V acc = compiler.mul_const(state[0], c.mds[i][0]);
            for (int j = 1; j < W; j++) acc = compiler.add(acc, compiler.mul_const(state[j], c.mds[i][j]));
            nx[i] = acc;
        }
        for (int i = 0; i < W; i++) state[i] = nx[i];
    }
}
// in-circuit hash of W - 1 inputs (Hasher::hash, hash.rs:123-135; Spec<F, ARITY>, plugins/arkworks/src/poseidon/mod.rs:225-322): state =
// (2^arity - 1, in[0] .. in[W - 2]), output = lane 0
template <class FrP, int W>
FpVar<FrP> hash(const Constants<FrP, W>& c, const FpVar<FrP>* in, R1CS<FrP>& compiler) {
    FpVar<FrP> state[W];
    state[0] = compiler.constant(zl::from_u64<FrP>(c.SPEC.tag));
    for (int i = 1; i < W; i++) state[i] = in[i - 1];
    permute<FrP, W>(c, state, compiler);
    return state[0];
}
// the arity-2 form the chain and the Merkle levels call: the W = 3 instance
template <class FrP>
FpVar<FrP> hash(const Constants<FrP>& c, const FpVar<FrP>& x, const FpVar<FrP>& y, R1CS<FrP>& compiler) {
    const FpVar<FrP> in[2] = {x, y};
    return hash<FrP, 3>(c, in, compiler);
}

// ---- the duplex-sponge authenticated cipher over the permutation (openzl-crypto/src/permutation/duplex.rs, sponge.rs; poseidon/encryption.rs) ----
// Rate W - 1, lanes 1 .. W - 1; lane 0 is never written.  The setup blocks are padded_chunks_with(key, rate, 0) followed by padded_chunks_with(header,
// rate, 0) (openzl-util/src/vec.rs:60-77): ALWAYS one last, zero-padded chunk per sequence, also when nothing is left over -- floor(K / rate) + 1 key blocks,
// floor(H / rate) + 1 header blocks.  Every block is added into the rate and the state permuted; a message block's ciphertext is the rate read BEFORE the
// permutation.  The tag is lane 1 after the last permutation.  Elements are Montgomery; the padding zeros are skipped, not added.
constexpr size_t duplex_setup_blocks(unsigned width, size_t key_len, size_t header_len) { return key_len / (width - 1) + 1 + header_len / (width - 1) + 1; }
template <class FrP, int W>
void duplex_setup(const Constants<FrP, W>& c, Fp<FrP> state[W], const Fp<FrP>* key, size_t key_len, const Fp<FrP>* header, size_t header_len) {
    constexpr size_t rate = W - 1;
    for (int part = 0; part < 2; part++) {
        const Fp<FrP>* src = part ? header : key;
        const size_t len = part ? header_len : key_len;
        for (size_t b = 0; b <= len / rate; b++) {
            for (size_t i = 0; i < rate && b * rate + i < len; i++) state[1 + i] = zl::add(state[1 + i], src[b * rate + i]);
            permute_native(c, state);
        }
    }
}
// text: blocks x rate elements, plaintext in, ciphertext out; state: the initial state in, left as the cipher leaves it; returns the tag
template <class FrP, int W>
Fp<FrP> duplex_encrypt(const Constants<FrP, W>& c, Fp<FrP> state[W], const Fp<FrP>* key, size_t key_len, const Fp<FrP>* header, size_t header_len, Fp<FrP>* text,
                       size_t blocks) {
    constexpr size_t rate = W - 1;
    duplex_setup(c, state, key, key_len, header, header_len);
    for (size_t j = 0; j < blocks; j++) {
        for (size_t i = 0; i < rate; i++) text[j * rate + i] = state[1 + i] = zl::add(state[1 + i], text[j * rate + i]);
        permute_native(c, state);
    }
    return state[1];
}
// text: ciphertext in, plaintext out; returns the COMPUTED tag, which the caller compares with the one it was given (Verify)
template <class FrP, int W>
Fp<FrP> duplex_decrypt(const Constants<FrP, W>& c, Fp<FrP> state[W], const Fp<FrP>* key, size_t key_len, const Fp<FrP>* header, size_t header_len, Fp<FrP>* text,
                       size_t blocks) {
    constexpr size_t rate = W - 1;
    duplex_setup(c, state, key, key_len, header, header_len);
    for (size_t j = 0; j < blocks; j++) {
        for (size_t i = 0; i < rate; i++) {
            const Fp<FrP> ct = text[j * rate + i];
            text[j * rate + i] = zl::sub(ct, state[1 + i]);
            state[1 + i] = ct;
        }
        permute_native(c, state);
    }
    return state[1];
}
// The cipher in circuit over a running state of W variables or constants: duplex_setup's and duplex_encrypt's block walk on variables.  `key` may be fresh
// witnesses (zl_circuit_poseidon_encrypt) or variables the circuit already holds (zl_circuit_hybrid_encrypt: the agreed point's coordinates); additions into
// the rate are linear and allocate nothing, so the only witnesses are the S-box records of the permutations, in execution order.  ct[j] receives the rate lane
// read before the permutation of message block j / rate; the state is left as the cipher leaves it: the tag is state[1].
template <class FrP, int W>
void duplex_encrypt_circuit(const Constants<FrP, W>& c, FpVar<FrP> state[W], const std::vector<FpVar<FrP>>& key, const std::vector<FpVar<FrP>>& header,
                            const std::vector<FpVar<FrP>>& text, std::vector<FpVar<FrP>>& ct, R1CS<FrP>& cs) {
    constexpr size_t rate = W - 1;
    for (int part = 0; part < 2; part++) {
        const std::vector<FpVar<FrP>>& src = part ? header : key;
        for (size_t b = 0; b <= src.size() / rate; b++) {
            for (size_t i = 0; i < rate && b * rate + i < src.size(); i++) state[1 + i] = cs.add(state[1 + i], src[b * rate + i]);
            permute<FrP, W>(c, state, cs);
        }
    }
    ct.resize(text.size());
    for (size_t j = 0; j < text.size() / rate; j++) {
        for (size_t i = 0; i < rate; i++) ct[j * rate + i] = state[1 + i] = cs.add(state[1 + i], text[j * rate + i]);
        permute<FrP, W>(c, state, cs);
    }
}
}  // namespace poseidon

// ---- the embedded twisted Edwards curve in circuit ----------------------------------------------------------------------------------------
// r1cs-std's affine twisted-Edwards variable (ark-r1cs-std groups/curves/twisted_edwards: AffineVar double / add) and its default double-and-add
// scalar_mul_le, RESTATED from the published formulas over this compiler -- as zl_edwards.h restates the curve constants.  It is NOT compared with arkworks
// matrices: the reference holds none.  a x^2 + y^2 = 1 + d x^2 y^2 with `a` a square and `d` not: both denominators below are non-zero for on-curve inputs,
// the law is complete and the identity is the ordinary point (0, 1).  Every quotient is a mul_equals: its value is a host division, its row a product.
//   double (x, y) -> (x3, y3): 5 rows, 5 witnesses, in this order
//       xy = x y    xx = x x    yy = y y    (a xx + yy) x3 = 2 xy    (2 - a xx - yy) y3 = yy - a xx
//   add (x1, y1) + (x2, y2): 6 rows, 6 witnesses, in this order
//       u = (y1 - a x1)(x2 + y2)    v0 = x1 y2    v1 = x2 y1    w = v0 v1    (1 + d w) x3 = v0 + v1    (1 - d w) y3 = u + a v0 - v1
//       (u + a v0 - v1 = y1 y2 - a x1 x2)
//   scalar_mul over `bits` bits b_0 .. b_{bits - 1} (Boolean witnesses, least significant first) of a point P whose coordinates are VARIABLES:
//       R_1 = (select(b_0, P.x, 0), select(b_0, P.y, 1)); for i = 1 .. bits - 1: M_i = double(M_{i-1}) with M_0 = P, T = R_i + M_i,
//       R_{i+1} = (select(b_i, T.x, R_i.x), select(b_i, T.y, R_i.y)): 13 rows and 13 witnesses a step, 2 in front.
//   The ladder does NOT start from the constant identity and add to it: a product by the constant 0 is a linear combination the full compiler folds and the
//   witness-only compiler does not (the konst note in R1CS::mul), and the rows of the two would stop lining up.  In the form above every operand of a
//   product is a variable, so R1CS::witness_only_compatible() holds.
namespace edwards {
template <class FrP>
struct Coeffs {
    Fp<FrP> a, d;  // Montgomery
};
template <class FrP>
struct PointVar {
    FpVar<FrP> x, y;
};
template <class FrP>
PointVar<FrP> double_point(const Coeffs<FrP>& k, const PointVar<FrP>& p, R1CS<FrP>& cs) {
    using F = Fp<FrP>;
    using V = FpVar<FrP>;
    const F m1 = R1CS<FrP>::minus_one();
    const V xy = cs.mul(p.x, p.y), xx = cs.mul(p.x, p.x), yy = cs.mul(p.y, p.y);
    const V axx = cs.mul_const(xx, k.a);
    const V den_x = cs.add(axx, yy), num_x = cs.add(xy, xy);
    const V x3 = cs.mul_equals(den_x, num_x, zl::mul(num_x.value, zl::inv(den_x.value)));
    const V den_y = cs.add_const(cs.mul_const(den_x, m1), zl::from_u64<FrP>(2)), num_y = cs.add(yy, cs.mul_const(axx, m1));
    const V y3 = cs.mul_equals(den_y, num_y, zl::mul(num_y.value, zl::inv(den_y.value)));
    return PointVar<FrP>{x3, y3};
}
template <class FrP>
PointVar<FrP> add_points(const Coeffs<FrP>& k, const PointVar<FrP>& p, const PointVar<FrP>& q, R1CS<FrP>& cs) {
    using F = Fp<FrP>;
    using V = FpVar<FrP>;
    const F m1 = R1CS<FrP>::minus_one();
    const V u = cs.mul(cs.add(p.y, cs.mul_const(p.x, zl::mul(k.a, m1))), cs.add(q.x, q.y));
    const V v0 = cs.mul(p.x, q.y), v1 = cs.mul(q.x, p.y), w = cs.mul(v0, v1);
    const V dw = cs.mul_const(w, k.d);
    const V den_x = cs.add_const(dw, F::one()), num_x = cs.add(v0, v1);
    const V x3 = cs.mul_equals(den_x, num_x, zl::mul(num_x.value, zl::inv(den_x.value)));
    const V den_y = cs.add_const(cs.mul_const(dw, m1), F::one()), num_y = cs.add(cs.add(u, cs.mul_const(v0, k.a)), cs.mul_const(v1, m1));
    const V y3 = cs.mul_equals(den_y, num_y, zl::mul(num_y.value, zl::inv(den_y.value)));
    return PointVar<FrP>{x3, y3};
}
// The scalar's side of a multiplication: `bits` Boolean witnesses b_0 .. (least significant first, one row each) of the words s_words, and the row
// sum 2^i b_i = s for a variable s the circuit already holds.  One decomposition may feed several ladders (zl_circuit_hybrid_encrypt: esk G and esk pk).
template <class FrP>
std::vector<FpVar<FrP>> scalar_bits(const FpVar<FrP>& s, const uint64_t* s_words, unsigned bits, R1CS<FrP>& cs) {
    using F = Fp<FrP>;
    std::vector<FpVar<FrP>> b(bits);
    for (unsigned i = 0; i < bits; i++) b[i] = cs.new_boolean_witness((s_words[i >> 6] >> (i & 63)) & 1);
    FpVar<FrP> sum = b[0];
    F pow2 = F::one();
    for (unsigned i = 1; i < bits; i++) {
        pow2 = zl::add(pow2, pow2);
        sum = cs.add(sum, cs.mul_const(b[i], pow2));
    }
    cs.enforce_equal(sum, s);
    return b;
}
// the ladder over given bits from a point whose coordinates are variables.  bits: the Boolean witnesses of the scalar, least significant first, at least one
template <class FrP>
PointVar<FrP> scalar_mul_le(const Coeffs<FrP>& k, const PointVar<FrP>& p, const std::vector<FpVar<FrP>>& bits, R1CS<FrP>& cs) {
    using F = Fp<FrP>;
    PointVar<FrP> r{cs.select(bits[0], p.x, cs.constant(F::zero())), cs.select(bits[0], p.y, cs.constant(F::one()))};
    PointVar<FrP> m = p;
    for (size_t i = 1; i < bits.size(); i++) {
        m = double_point(k, m, cs);
        const PointVar<FrP> t = add_points(k, r, m, cs);
        r = PointVar<FrP>{cs.select(bits[i], t.x, r.x), cs.select(bits[i], t.y, r.y)};
    }
    return r;
}
}  // namespace edwards

// ---- pairing-engine configs ---------------------------------------------------------------------------------------------------
struct Bls12_381 {
    using FrP = BLS12_381_Fr;
    using G1 = BlsG1;
    using G2 = BlsG2;
    using PairingP = BLS12_381_Pairing;
    static constexpr zl_curve_t curve = ZL_BLS12_381;
};
struct Bn254 {
    using FrP = BN254_Fr;
    using G1 = BnG1;
    using G2 = BnG2;
    using PairingP = BN254_Pairing;
    static constexpr zl_curve_t curve = ZL_BN254;
};

// ---- Groth16<E>: ProofSystem (groth16.rs:405-467) -------------------------------------------------------------------------------
struct Error {
    int code;  // the reference's Error is an opaque unit struct (groth16.rs:35-45); the code is extra, for diagnostics
};
template <class T>
struct Result {
    bool ok;
    T value;
    Error error;
};

template <class FrP> struct R1csExport;
template <class E>
struct Groth16 {
    using FrP = typename E::FrP;
    using F = Fp<FrP>;
    using Compiler = R1CS<FrP>;
    struct Trapdoor { F alpha, beta, gamma, delta, tau; };  // canonical
    struct ProvingContext {                                 // ProvingContext<E>(pub ProvingKey<E>) groth16.rs:127-140
        zl_ctx* ctx = nullptr;
        uint64_t a_query = 0, b_g1_query = 0, h_query = 0, l_query = 0, b_g2_query = 0;
        // device-resident constraint matrices (static per circuit): uploaded by compile; a context decoded from bytes does not know its
        // circuit, so the first prove() uploads them and BINDS the context to that circuit (hence mutable: the first prove of a decoded
        // context mutates it, so it must not race with another prove on the same context; every later prove is read-only).
        // circuit_digest = R1CS::structure_digest() of the bound circuit: a compiler with another fingerprint is refused.
        mutable uint64_t r1cs = 0;
        mutable size_t n_constraints = 0;
        mutable uint64_t circuit_digest = 0;
        mutable bool witness_only_ok = true;  // the bound circuit folds constants alike in both compiler modes (R1CS::witness_only_compatible)
        std::vector<uint64_t> alpha_g1, beta_g1, delta_g1, beta_g2, delta_g2;
        size_t n_instance = 0, n_witness = 0, domain_size = 0;
        Trapdoor trapdoor;  // kept ONLY so tests can recompute proofs in the exponent; a real setup drops it
        bool has_trapdoor = false;  // false for a context decoded from bytes
    };
    struct VerifyingContext {  // ark_groth16::VerifyingKey (the reference holds it prepared, groth16.rs:181-186); canonical affine points
        std::vector<uint64_t> alpha_g1, beta_g2, gamma_g2, delta_g2;
        std::vector<uint64_t> gamma_abc_g1;  // n_instance points, index 0 pairs with the constant ONE
        std::vector<F> gamma_abc_exponents;  // discrete logs, kept for exponent checks in tests
    };
    using Input = std::vector<F>;
    using Proof = zl_g16_proof;

    static Compiler context_compiler() { return Compiler::for_contexts(); }  // groth16.rs:418-420
    static Compiler proof_compiler() { return Compiler::for_proofs(); }      // groth16.rs:423-425
    // `exported`: the CSR export of `compiler` when the caller already holds one (the C hooks do): saves rebuilding it for the matrix upload
    static Result<std::pair<ProvingContext, VerifyingContext>> compile(zl_ctx* ctx, const Compiler& compiler, SplitMix64& rng,
                                                                        const R1csExport<FrP>* exported = nullptr);
    // lane: the ctx the proof runs on -- the context's own (default) or a fork of it (zl_ctx_fork): N host threads, one lane each, prove side by side over
    // ONE device-resident key, as N threads may share the reference's `&ProvingContext`.  A context decoded from bytes is bound (first proof) on its own ctx.
    static Result<Proof> prove(const ProvingContext& context, const Compiler& compiler, SplitMix64& rng, F* r_out = nullptr, F* s_out = nullptr,
                               zl_ctx* lane = nullptr);
    // verify (groth16.rs:459-466): e(A, B) == e(alpha, beta) e(sum_i x_i gamma_abc_i, gamma) e(C, delta); input = public inputs (canonical)
    static Result<bool> verify(const VerifyingContext& vk, const Input& input, const Proof& proof);
    static void release(ProvingContext& context);
    // Wire format of ProvingContext<E> (codec::Encode / Decode, groth16.rs:142-179): ark_groth16::ProvingKey<E> written with
    // serialize_unchecked = the uncompressed form (zl_serialize.h).  The key carries its VerifyingKey, so encode takes both halves of
    // compile()'s result and decode returns both.  decode uploads the five queries (flags: ZL_CHECK verifies every point on the
    // device) and builds the same window tables as compile; like the reference's deserialize_unchecked it trusts the bytes otherwise.
    static Result<std::vector<uint8_t>> encode(const ProvingContext& context, const VerifyingContext& vk);
    static Result<std::pair<ProvingContext, VerifyingContext>> decode(zl_ctx* ctx, const uint8_t* bytes, size_t len, unsigned flags = 0);
    // ark_groth16::VerifyingKey<E>::serialize (compressed): alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1
    static std::vector<uint8_t> encode_verifying_key(const VerifyingContext& vk);
    static int build_window_tables(const ProvingContext& context);  // the per-query tables of a large key (compile and decode)
};

// CSR export of a compiler (what ark hands to the prover as ConstraintMatrices + assignments)
template <class FrP>
struct R1csExport {
    std::vector<uint32_t> ptr[3], col[3];
    std::vector<uint64_t> val[3];
    std::vector<uint64_t> assignment;
    zl_r1cs view{};
    void build(const R1CS<FrP>& cs);
};

}  // namespace openzl
