"""GPU parity of zl_ntt on every pass plan and table fallback of its host driver (zl_ntt.hip: ntt_plan / ntt_run_t), bit-exact against the CPU oracle.

test_gpu_ntt.py compares with the oracle at BASE_SIZES only.  Which code a transform reaches depends on its size (number of passes, odd pass sizes, row
tables or per-tile row twiddles, a tabulated or an on-the-fly last pass), on the table budget of the ctx, on ctx->ntt_fit_beside and on the representation
flags; every one of those choices is pinned here against a reference.  tests/test_ntt_plan.py (CPU) holds the plan itself and checks that the size lists
below cover every distinct tuple of pass sizes.

All comparisons are exact: integers mod r.  The threaded oracle entry (Montgomery in / out) is fed canonical limbs: the transform is linear, so the words x
read as the Montgomery forms of x / R come back as NTT(x / R) R = NTT(x) (pinned in test_ntt_plan.py).  The same holds for the kernel, whose data keeps the
caller's form."""
import numpy as np
import pytest

import oracle_lib as ol
import test_gpu_ntt
from oracle_lib import po

pytestmark = pytest.mark.gpu
CURVES = [po.BLS12_381, po.BN254]
VARIANTS = [(False, False), (True, False), (False, True), (True, True)]  # (inverse, coset)
VARIANT_IDS = ["fwd", "inv", "coset_fwd", "coset_inv"]
# the sizes test_gpu_ntt.test_ntt_matches_oracle holds (read from its parametrisation, so the two lists cannot drift apart)
BASE_SIZES = sorted(next(m.args[1] for m in test_gpu_ntt.test_ntt_matches_oracle.pytestmark if m.name == "parametrize" and m.args[0] == "log_n"))
ORACLE_SIZES = [n for n in range(25) if n not in BASE_SIZES]  # all four variants, both curves
# 2^25 / 2^26 (2 GiB per vector, ~10 s of oracle per transform): both curves at each size, every variant once per curve across the two
REDUCED_VARIANTS = {
    25: {"bls12_381": [(False, False), (True, True)], "bn254": [(False, False), (True, True)]},
    26: {"bls12_381": [(True, False), (False, True)], "bn254": [(True, False), (False, True)]},
}
DEVICE_CASES = [(27, po.BLS12_381), (28, po.BN254)]  # beyond the oracle's reach: device-resident data, closed-form references
ORACLE_THREADS = 16
THREADED_FROM = 19  # log_n from which the threaded oracle entry is used
CACHE_UP_TO = 22    # expected values up to this size are kept for the other parts of this module (128 MiB each at 2^22)
_EXPECTED = {}


def _fid(curve):
    return 2 if curve.cid == 1 else 4


def _fast_scalars(curve, n, seed):
    """n scalars below 2^(bits - 1) <= r: uniform 64-bit limbs with the top limb masked (no rejection loop: 2^26 elements in about a second)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    out[:, 3] &= np.uint64((1 << (curve.fr.bits - 193)) - 1)
    return out


def _input(curve, log_n, seed=None):
    seed = 7000 + log_n if seed is None else seed
    return ol.random_scalars(curve, 1 << log_n, seed) if log_n < THREADED_FROM else _fast_scalars(curve, 1 << log_n, seed)


def _oracle(curve, x, inverse, coset):
    log_n = int(x.shape[0]).bit_length() - 1
    if log_n < THREADED_FROM:
        return ol.oracle_ntt(curve, x, inverse=inverse, coset=coset, mont=False)
    return ol.oracle_ntt_timed(curve, x, inverse=inverse, coset=coset, threads=ORACLE_THREADS)[0]


def _expected(curve, log_n, inverse, coset, seed=None):
    """the oracle transform of _input(curve, log_n, seed); shared between the parts of this module up to 2^CACHE_UP_TO"""
    seed = 7000 + log_n if seed is None else seed
    key = (curve.name, log_n, inverse, coset, seed)
    if key in _EXPECTED:
        return _EXPECTED[key]
    exp = _oracle(curve, _input(curve, log_n, seed), inverse, coset)
    if log_n <= CACHE_UP_TO:
        _EXPECTED[key] = exp
    return exp


def _same(got, exp, what=""):
    """bit-exact equality of two (n, 4) limb arrays; a mismatch names the first differing element (which pass owns it follows from the plan)"""
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if np.array_equal(got, exp):
        return
    bad = np.nonzero((got != exp).any(axis=1))[0]
    i = int(bad[0])
    pytest.fail(f"{what}: {bad.size} of {got.shape[0]} elements differ, first at index {i} (last at {int(bad[-1])}): got {ol.limbs_to_ints(got[i:i + 1])[0]:#x}, expected {ol.limbs_to_ints(exp[i:i + 1])[0]:#x}")


def _check_against_oracle(be, curve, log_n, inverse, coset, what=""):
    x = _input(curve, log_n)
    got = be.ntt(curve.cid, x, inverse=inverse, coset=coset, mont=False)
    del x
    _same(got, _expected(curve, log_n, inverse, coset), f"{what} {curve.name} 2^{log_n} inverse={inverse} coset={coset}")


def _to_mont(curve, a):
    out = np.zeros_like(a)
    assert ol.lib().zlo_field_to_mont(_fid(curve), ol.p64(np.ascontiguousarray(a).reshape(-1)), ol.p64(out.reshape(-1)), a.shape[0]) == 0
    return out


def _to_ints(a):
    b = np.ascontiguousarray(a, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(len(b) // 32)]


def _dev(x):
    import torch

    return torch.from_numpy(x.view(np.int64).copy()).cuda()


def _host(d):
    return d.cpu().numpy().view(np.uint64)


# ------------------------------------------------------------------------------------------------ 1. every plan against the oracle
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("log_n", ORACLE_SIZES)
@pytest.mark.parametrize("inverse,coset", VARIANTS, ids=VARIANT_IDS)
def test_every_plan_matches_oracle(backend, curve, log_n, inverse, coset):
    """one pass with s = n (7, 9: a half round after the two-stage rounds; 9: s > 8), two passes [8,6] [8,7], every three-pass plan up to [8,8,8]"""
    _check_against_oracle(backend, curve, log_n, inverse, coset)


@pytest.mark.parametrize("log_n,curve,inverse,coset", [(n, c, inv, cs) for n in sorted(REDUCED_VARIANTS) for c in CURVES for inv, cs in REDUCED_VARIANTS[n][c.name]],
                         ids=lambda v: getattr(v, "name", str(v)))
def test_four_pass_plans_match_oracle(backend, log_n, curve, inverse, coset):
    """2^25 [6,6,6,7] and 2^26 [8,6,6,6].  At 2^26 the last-pass table wants the whole default budget and the two row tables come first, so the last pass
    combines its twiddles on the fly (last_tw == nullptr) under production settings."""
    _check_against_oracle(backend, curve, log_n, inverse, coset)


# ------------------------------------------------------------------------------------------------ 3. table budget, fallbacks, eviction
def _fresh_backend():
    from openzl_amd import Backend

    return Backend(0)


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("log_n", [12, 17, 20, 22])
def test_budget_zero_no_tables_at_all(monkeypatch, curve, log_n):
    """ZL_TUNE_NTT_LAST_MB=0 on a fresh ctx: neither the last-pass table nor any row table can be built, so the last pass combines on the fly and every
    middle pass forms its row twiddles per tile in LDS (sh_row, the larger dynamic LDS request): [6,6], [6,6,5], [8,6,6], [8,8,6]"""
    monkeypatch.setenv("ZL_TUNE_NTT_LAST_MB", "0")
    be = _fresh_backend()
    try:
        for inverse, coset in VARIANTS:
            _check_against_oracle(be, curve, log_n, inverse, coset, "budget 0")
    finally:
        be.close()


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("budget_mb", [32, 33])
def test_budget_row_table_without_last_table(monkeypatch, curve, budget_mb):
    """2^20 = [8,6,6].  The driver allocates in pass order: the pass-2 row table first, (32 B << (8 + 6)) = 512 KiB, then the last-pass table,
    2^20 * 32 B = 32 MiB.  Budget 32 MiB: the last table passes `want <= table_budget` by equality, but 0.5 + 32 > 32 beside the row table, so the row
    table is used and the last pass combines on the fly -- what 2^26 meets under the default budget (2 GiB wanted of 2 GiB, row tables first).  Budget
    33 MiB: 0.5 + 32 <= 33, both are built."""
    monkeypatch.setenv("ZL_TUNE_NTT_LAST_MB", str(budget_mb))
    be = _fresh_backend()
    try:
        for inverse, coset in VARIANTS:
            _check_against_oracle(be, curve, 20, inverse, coset, f"budget {budget_mb}")
    finally:
        be.close()


def test_budget_eviction_and_rebuild(monkeypatch):
    """Budget 34 MiB holds the tables of one 2^20 key (0.5 + 32 MiB) and no second one.  forward 2^20 builds its two tables; inverse 2^20 (another key) fits
    its row table (33 <= 34) and evicts the forward key for its last table; forward 2^18 BN254 ([6,6,6]: 128 KiB + 8 MiB) evicts the inverse key; forward 2^20
    again rebuilds what was freed and evicts the BN254 key: make_room's victim choice, the stream drain, hipFree and the rebuild on next use"""
    monkeypatch.setenv("ZL_TUNE_NTT_LAST_MB", "34")
    be = _fresh_backend()
    try:
        _check_against_oracle(be, po.BLS12_381, 20, False, False, "eviction step 1")
        _check_against_oracle(be, po.BLS12_381, 20, True, False, "eviction step 2")
        _check_against_oracle(be, po.BN254, 18, False, False, "eviction step 3")
        _check_against_oracle(be, po.BLS12_381, 20, False, False, "eviction step 4")
        _check_against_oracle(be, po.BLS12_381, 20, True, False, "eviction step 5")
    finally:
        be.close()


def test_default_budget_interleaved_sweep():
    """one ctx, default budget, 2^16 .. 2^24 x both directions x both curves in a shuffled order: the twiddle-cache key and the LRU clock see a realistic
    mix (1 GiB of last-pass tables at 2^24 alone, so the 2-GiB budget evicts along the way)"""
    cases = [(log_n, curve, inverse) for log_n in range(16, 25) for curve in CURVES for inverse in (False, True)]
    order = np.random.Generator(np.random.PCG64(11)).permutation(len(cases))
    be = _fresh_backend()
    try:
        for i in order:
            log_n, curve, inverse = cases[int(i)]
            _check_against_oracle(be, curve, log_n, inverse, False, "sweep")
    finally:
        be.close()


# ------------------------------------------------------------------------------------------------ 4. the MINB = 5 instantiations
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("log_n", [8, 11, 14, 17, 20, 22, 24])
def test_fit_beside_instantiations_match_oracle(backend, curve, log_n):
    """ctx->ntt_fit_beside selects k_ntt_pass28<.., MINB = 5> (96 registers, spills): otherwise reached only inside a whole Groth16 proof"""
    from openzl_amd.backend import hook_ntt_fit_beside

    old = hook_ntt_fit_beside(backend, True)
    try:
        assert hook_ntt_fit_beside(backend, True) is True
        for inverse, coset in VARIANTS:
            _check_against_oracle(backend, curve, log_n, inverse, coset, "fit_beside")
    finally:
        hook_ntt_fit_beside(backend, old)
    assert hook_ntt_fit_beside(backend, old) == old


def _batch_against_oracle(be, curve, log_n, flags, count, stride, seed):
    """zl_ntt_batch_dev on `count` vectors `stride` elements apart against the oracle transform of each; the gap words stay untouched.  With ZL_MONT (or no
    representation flag) the kernel converts nothing, so the expected limbs are the oracle's on the same limbs (linearity, see the module docstring)."""
    import torch
    from openzl_amd.backend import ZL_COSET, ZL_INVERSE

    n = 1 << log_n
    x = (ol.random_scalars if log_n < THREADED_FROM else _fast_scalars)(curve, count * stride, seed).reshape(count, stride, 4)
    d = _dev(x.reshape(-1, 4))
    be.ntt_batch_dev(curve.cid, d.data_ptr(), log_n, flags, count, stride)
    torch.cuda.synchronize()
    got = _host(d).reshape(count, stride, 4)
    for v in range(count):
        exp = _oracle(curve, np.ascontiguousarray(x[v, :n]), bool(flags & ZL_INVERSE), bool(flags & ZL_COSET))
        _same(got[v, :n], exp, f"batch {curve.name} 2^{log_n} flags={flags} count={count} stride={stride} vector {v}")
    assert (got[:, n:] == x[:, n:]).all(), "gap words changed"


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("log_n", [8, 14, 17, 20])
def test_fit_beside_batch_matches_oracle(backend, curve, log_n):
    from openzl_amd.backend import ZL_COSET, ZL_INVERSE, ZL_MONT, hook_ntt_fit_beside

    old = hook_ntt_fit_beside(backend, True)
    try:
        for flags in (ZL_MONT, ZL_MONT | ZL_INVERSE | ZL_COSET):
            _batch_against_oracle(backend, curve, log_n, flags, 3, (1 << log_n) + 8, 5100 + log_n)
    finally:
        hook_ntt_fit_beside(backend, old)


# ------------------------------------------------------------------------------------------------ 5. representation flags, one at a time
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("log_n", [0, 1, 9, 13, 19])
def test_representation_flags_one_at_a_time(backend, curve, log_n):
    """ZL_MONT_IN alone (from_mont on the last pass), ZL_MONT_OUT alone (to_mont on pass 1), ZL_MONT, none -- each with every direction / coset combination:
    expected = the oracle transform with the input / output converted by the oracle's own to_mont"""
    import torch
    from openzl_amd.backend import ZL_COSET, ZL_INVERSE, ZL_MONT, ZL_MONT_IN, ZL_MONT_OUT, BackendError

    x = _input(curve, log_n, 8100 + log_n)
    xm = _to_mont(curve, x)
    for inverse, coset in VARIANTS:
        exp = _oracle(curve, x, inverse, coset)
        exp_m = _to_mont(curve, exp)
        for rep in (ZL_MONT_IN, ZL_MONT_OUT, ZL_MONT, 0):
            flags = rep | (ZL_INVERSE if inverse else 0) | (ZL_COSET if coset else 0)
            mont_in, mont_out = bool(rep & (ZL_MONT | ZL_MONT_IN)), bool(rep & (ZL_MONT | ZL_MONT_OUT))
            d = _dev(xm if mont_in else x)
            if log_n == 0 and mont_in != mont_out:
                with pytest.raises(BackendError):  # one element: the identity, which cannot convert
                    backend.ntt_dev_flags(curve.cid, d.data_ptr(), log_n, flags)
                continue
            backend.ntt_dev_flags(curve.cid, d.data_ptr(), log_n, flags)
            torch.cuda.synchronize()
            _same(_host(d), exp_m if mont_out else exp, f"{curve.name} 2^{log_n} flags={flags}")
            if log_n == 0:
                assert (_host(d) == (xm if mont_in else x)).all()


# ------------------------------------------------------------------------------------------------ 6. structured and extreme inputs
def _const(n, value):
    return np.tile(ol.ints_to_limbs([value], 4), (n, 1))


def _structured_inputs(curve, log_n):
    """(name, input, closed form of the plain forward transform or None)"""
    n, r = 1 << log_n, curve.fr.p
    w = po.domain_root(curve, log_n)
    zero = np.zeros((n, 4), dtype=np.uint64)

    def at(pairs):
        a = zero.copy()
        for i, v in pairs:
            a[i] = ol.ints_to_limbs([v % r], 4)[0]
        return a

    yield "zero", zero, zero
    yield "all_r_minus_1", _const(n, r - 1), at([(0, -n)])                     # -sum_j w^(jk) = -n at k = 0, 0 elsewhere
    yield "all_one", _const(n, 1), at([(0, n)])
    # delta_k -> w^(jk) at every j: pins the twiddle index of every element.  The root table T[e] = w^e is the oracle's transform of delta_1, itself checked
    # against Python's pow at a few exponents; w^(jk) = T[jk mod n] is then a gather
    table = _oracle(curve, at([(1, 1)]), False, False)
    rng = np.random.Generator(np.random.PCG64(600 + log_n))
    for e in [0, 1, 2, n // 2, n - 1] + [int(v) for v in rng.integers(0, n, 6)]:
        assert _to_ints(table[e:e + 1])[0] == pow(w, e, r)
    j = np.arange(n, dtype=np.int64)
    for k in [0, 1, n // 2, n - 1] + [int(v) for v in rng.integers(2, n - 1, 2)]:
        yield f"delta_{k}", at([(k, 1)]), table[(j * k) & (n - 1)]
    alt = zero.copy()
    alt[1::2] = ol.ints_to_limbs([r - 1], 4)[0]
    # -sum_(j odd) w^(jk) = -w^k sum_i w^(2ik): -(n/2) at k = 0, -(n/2) w^(n/2) = +n/2 at k = n/2, 0 elsewhere
    yield "alternating_0_r_minus_1", alt, at([(0, -(n // 2)), (n // 2, n // 2)])
    half = zero.copy()
    half[:n // 2] = ol.ints_to_limbs([r - 1], 4)[0]
    yield "first_half_r_minus_1", half, None


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("log_n", [10, 15, 19, 23])
def test_structured_and_extreme_inputs(backend, curve, log_n):
    """the values the lazily reduced passes' bounds are tight for (all r - 1, worst-case sums on one butterfly side) and inputs whose transform is known in
    closed form at every index, all four variants against the oracle and the plain forward transform against the closed form as well"""
    for name, x, closed in _structured_inputs(curve, log_n):
        for inverse, coset in VARIANTS:
            what = f"{name} {curve.name} 2^{log_n} inverse={inverse} coset={coset}"
            got = backend.ntt(curve.cid, x, inverse=inverse, coset=coset, mont=False)
            _same(got, _oracle(curve, x, inverse, coset), what)
            if name == "zero":
                assert not got.any(), what
            if closed is not None and not inverse and not coset:
                _same(got, closed, what + " (closed form)")


# ------------------------------------------------------------------------------------------------ 7. batch against the oracle
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("log_n", [9, 15, 19])
@pytest.mark.parametrize("count", [1, 2, 5])
@pytest.mark.parametrize("gap", [0, 8], ids=["stride_n", "stride_n_plus_8"])
def test_batch_matches_oracle(backend, curve, log_n, count, gap):
    from openzl_amd.backend import ZL_COSET, ZL_INVERSE, ZL_MONT

    for flags in (ZL_MONT, ZL_MONT | ZL_INVERSE | ZL_COSET):
        _batch_against_oracle(backend, curve, log_n, flags, count, (1 << log_n) + gap, 9100 + 16 * log_n + count)


# ------------------------------------------------------------------------------------------------ 2. device-resident sizes (these run last, one check per test)
# 2^27 [8,6,6,7]: the `n <= 26` gate keeps the last pass on the fly by design.  2^28 [8,8,6,6]: the third pass has S_prev + s = 22 > 20, so no row table:
# its row twiddles are formed per tile in LDS; BN254's two-adicity limit (the root-squaring loop of ntt_tables runs zero times).
SMALL_LOG = 20


def _device_need(log_n, vectors):
    """bytes: `vectors` 32-byte vectors held by the test + the driver's 36-byte scratch elements + a 4-byte-per-element comparison result + 1 GiB of slack"""
    return (1 << log_n) * (32 * vectors + 36 + 4) + (1 << 30)


def _require_device_memory(log_n, vectors):
    import torch

    torch.cuda.empty_cache()
    free, _total = torch.cuda.mem_get_info()
    need = _device_need(log_n, vectors)
    if free < need:
        pytest.skip(f"2^{log_n} needs {need} bytes of free device memory, torch.cuda.mem_get_info() reports {free}")


def _device_random(curve, n, seed):
    """(n, 4) int64 on the device, every value below 2^(bits - 1) <= r (top limb masked)"""
    import torch

    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 4), dtype=torch.int64, device="cuda", generator=g)
    x[:, 3] &= (1 << (curve.fr.bits - 193)) - 1
    return x


def _device_same(got, exp, what):
    import torch

    eq = got == exp
    if bool(eq.all()):
        return
    bad = torch.nonzero(~eq.reshape(-1, 4).all(dim=1))
    pytest.fail(f"{what}: {bad.shape[0]} elements differ, first at index {int(bad[0])}, last at {int(bad[-1])}")


@pytest.mark.parametrize("log_n,curve", DEVICE_CASES, ids=lambda v: getattr(v, "name", str(v)))
def test_device_resident_periodic_input(backend, log_n, curve):
    """x[j] != 0 only at multiples of 2^(n-m), dense x' there: X[k] = NTT_m(x')[k mod 2^m] at EVERY k -- all 2^n outputs against the tiled oracle transform"""
    import torch

    _require_device_memory(log_n, 1)
    n, m = 1 << log_n, 1 << SMALL_LOG
    xs = _input(curve, SMALL_LOG, 2700 + log_n)
    exp = _dev(_oracle(curve, xs, False, False))
    x = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    x[::n // m] = _dev(xs)
    torch.cuda.synchronize()  # the transform runs on the ctx's own stream: torch's work on the data has to be complete
    backend.ntt_dev_flags(curve.cid, x.data_ptr(), log_n, 0)
    torch.cuda.synchronize()
    _device_same(x.view(n // m, m, 4), exp.unsqueeze(0), f"periodic {curve.name} 2^{log_n}")


@pytest.mark.parametrize("log_n,curve", DEVICE_CASES, ids=lambda v: getattr(v, "name", str(v)))
def test_device_resident_low_support_coset(backend, log_n, curve):
    """x[j] != 0 only for j < 2^m: X[k 2^(n-m)] = cosetNTT_m(x')[k] (same generator) -- that stride of outputs against the oracle, and Horner's evaluation
    at g w^k in Python integers at indices off the stride"""
    import torch
    from openzl_amd.backend import ZL_COSET

    _require_device_memory(log_n, 1)
    n, m = 1 << log_n, 1 << SMALL_LOG
    xs = _input(curve, SMALL_LOG, 2800 + log_n)
    exp = _dev(_oracle(curve, xs, False, True))
    x = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    x[:m] = _dev(xs)
    torch.cuda.synchronize()
    backend.ntt_dev_flags(curve.cid, x.data_ptr(), log_n, ZL_COSET)
    torch.cuda.synchronize()
    _device_same(x[::n // m], exp, f"low support {curve.name} 2^{log_n}")
    r, w, g = curve.fr.p, po.domain_root(curve, log_n), curve.fr_generator
    coeffs = _to_ints(xs)
    rng = np.random.default_rng(log_n)
    for k in [1, n - 1, n // 2 + 1] + [int(v) | 1 for v in rng.integers(0, n, 3)]:
        pt = g * pow(w, k, r) % r
        acc = 0
        for cf in reversed(coeffs):
            acc = (acc * pt + cf) % r
        assert _to_ints(_host(x[k:k + 1]))[0] == acc, k


@pytest.mark.parametrize("log_n,curve", DEVICE_CASES, ids=lambda v: getattr(v, "name", str(v)))
def test_device_resident_dense_round_trip(backend, log_n, curve):
    """random dense input: forward then inverse, and coset forward then coset inverse, give the input back bit for bit"""
    import torch
    from openzl_amd.backend import ZL_COSET, ZL_INVERSE

    _require_device_memory(log_n, 2)
    n = 1 << log_n
    x = _device_random(curve, n, 2900 + log_n)
    x0 = x.clone()
    torch.cuda.synchronize()  # (the generator and the copy run on torch's stream, the transform on the ctx's)
    for cs in (0, ZL_COSET):
        backend.ntt_dev_flags(curve.cid, x.data_ptr(), log_n, cs)
        torch.cuda.synchronize()
        assert not torch.equal(x[:4096], x0[:4096])
        backend.ntt_dev_flags(curve.cid, x.data_ptr(), log_n, cs | ZL_INVERSE)
        torch.cuda.synchronize()
        _device_same(x, x0, f"round trip {curve.name} 2^{log_n} coset={bool(cs)}")
