"""Every launch geometry of the device Miller-product driver (miller_product / run() of csrc/zl_pairing_dev.hip) at tens of pairs: ZL_TUNE_PAIR_GROUPS
lowers the groups per launch (pairs then share a group, the launch pads to G * ng lanes and k_pd_prod folds the group values), ZL_TUNE_PAIR_SET the pairs
per launch set (and, being set, the reject-path chunk of zl_groth16_verify_batch to set / 4 proofs).  The workload reaches these branches only at thousands
of pairs; here they run with the 128-bit scalars of the batch verifier, with points at infinity, and under the batch verifier itself.  Expected values come
from the host: products of single host pairings in Python Fq12 arithmetic, the host lock-step multi-pairing over oracle points, the bilinear closed form,
the host batch verifier.  Every comparison is exact.  Each test computes G, ng and npad by the driver's formula and asserts the property it is there for,
so a change of the formula fails the test instead of emptying it; the default geometry runs once at 32 CU + 1 pairs with no knob."""
import os

import numpy as np
import pytest

import groth16_util as gu
import oracle_lib as ol
from oracle_lib import po
from openzl_amd import ZL_G1, ZL_G2, Circuit, Groth16Keys, pairing
from openzl_amd.backend import hook_pairing_product, hook_pairing_product_scaled, hook_verify_batch_host
from test_gpu_verify_batch_reject import HOST_ONLY, _tamper

pytestmark = pytest.mark.gpu

CURVES = [po.BLS12_381, po.BN254]
ONE = [1] + [0] * 11
POOL = 65
MAX_PAIRS = 1 << 16
KNOBS = ("ZL_TUNE_PAIR_GROUPS", "ZL_TUNE_PAIR_SET", "ZL_TUNE_FEXP_DEV_MIN", "ZL_TUNE_FEXP_CHUNK")


def _with_env(knobs, fn):
    """run fn with exactly the given knobs of KNOBS set (the others unset), then restore the environment"""
    assert set(knobs) <= set(KNOBS)
    old = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            if k in knobs:
                os.environ[k] = str(knobs[k])
            else:
                os.environ.pop(k, None)
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _env(groups=None, pair_set=None, dev_min=None):
    e = {}
    if groups is not None:
        e["ZL_TUNE_PAIR_GROUPS"] = groups
    if pair_set is not None:
        e["ZL_TUNE_PAIR_SET"] = pair_set
    if dev_min is not None:
        e["ZL_TUNE_FEXP_DEV_MIN"] = dev_min
    return e


def _cu_count():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _geometry(m, target):
    """the driver's launch geometry of one set of m pairs: (G pairs per group, ng groups, npad lanes)"""
    G = (m + target - 1) // target
    ng = (m + G - 1) // G
    return G, ng, G * ng


def _sets(n, target, pair_set=MAX_PAIRS):
    """(first, m, G, ng, npad) of every launch set of an n-pair product"""
    pair_set = min(max(pair_set, 1), MAX_PAIRS)
    return [(first, min(pair_set, n - first)) + _geometry(min(pair_set, n - first), target) for first in range(0, n, pair_set)]


def _prod_levels(ng):
    """launches of k_pd_prod that fold ng group values, 16 per group of lanes and level"""
    levels = 0
    while ng > 1:
        ng, levels = (ng + 15) // 16, levels + 1
    return levels


class Pool:
    """65 pairs (a_i G1, b_i G2) with their single host pairings"""

    def __init__(self, curve):
        self.curve = curve
        self.a = ol.limbs_to_ints(ol.random_scalars(curve, POOL, 11))
        self.b = ol.limbs_to_ints(ol.random_scalars(curve, POOL, 12))
        self.P = ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs(self.a, 4))
        self.Q = gu.g2_mul_gen(curve, self.b)
        self.ctx = po.Fq12Ctx(curve)
        self.single = [ol.limbs_to_ints(pairing(curve.cid, self.P[i], self.Q[i])) for i in range(POOL)]

    def product(self, idx):
        """the Python Fq12 product of the single host pairings of the pool's pairs idx"""
        acc = ONE
        for i in idx:
            acc = self.ctx.mul(acc, self.single[i])
        return acc


_POOLS = {}


@pytest.fixture(params=CURVES, ids=lambda c: c.name)
def pool(request):
    curve = request.param
    if curve.cid not in _POOLS:  # computed once per curve, never modified
        _POOLS[curve.cid] = Pool(curve)
    return _POOLS[curve.cid]


def _bilinear(backend, curve, n, seed):
    """n device-generated pairs (a_i G1, b_i G2) and the closed form e((sum a_i b_i) G1, G2) of their product"""
    a = ol.random_scalars(curve, n, seed)
    b = ol.random_scalars(curve, n, seed + 1)
    h1 = backend.bases_generate(curve.cid, a, group=ZL_G1)
    h2 = backend.bases_generate(curve.cid, b, group=ZL_G2)
    try:
        P, Q = backend.bases_download(h1), backend.bases_download(h2)
    finally:
        backend.bases_free(h1)
        backend.bases_free(h2)
    s = sum(x * y for x, y in zip(ol.limbs_to_ints(a), ol.limbs_to_ints(b))) % curve.fr.p
    exp = pairing(curve.cid, ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs([s], 4))[0], gu.g2_mul_gen(curve, [1])[0])
    return P, Q, exp


# ---- a. pairs share a group, the launch pads, k_pd_prod folds the groups ------------------------------------------------------------------------------
SHARED = [
    # n, t, G, ng, npad, what the case is there for
    (2, 1, 2, 1, 2, "one group, no pad"),
    (3, 2, 2, 2, 4, "one pad"),
    (7, 3, 3, 3, 9, "pad = G - 1"),
    (64, 5, 13, 5, 65, "ng no multiple of 4"),
    (65, 4, 17, 4, 68, "more pairs per group than k_pd_prod folds per level"),
    (33, 17, 2, 17, 34, "two k_pd_prod levels with a pad"),
    (65, 64, 2, 33, 66, "two k_pd_prod levels with a pad"),
]


@pytest.mark.parametrize("n,t,G,ng,npad,what", SHARED, ids=lambda v: str(v).replace(" ", "_"))
def test_shared_padded_reduced_products(backend, pool, n, t, G, ng, npad, what):
    assert _geometry(n, t) == (G, ng, npad) and G > 1 and n > t
    assert _geometry(n, 32 * _cu_count())[0] == 1  # the same call with no knob is the geometry the suite has always run
    if what == "one group, no pad":
        assert ng == 1 and npad == n
    elif what == "one pad":
        assert npad == n + 1
    elif what == "pad = G - 1":
        assert npad - n == G - 1 and G > 2
    elif what == "ng no multiple of 4":
        assert ng % 4 and npad > n
    elif what == "more pairs per group than k_pd_prod folds per level":
        assert G > 16 and npad - n > 1
    else:
        assert _prod_levels(ng) == 2 and npad > n
    curve, P, Q = pool.curve, pool.P[:n], pool.Q[:n]
    got = _with_env(_env(groups=t), lambda: backend.pairing_product(curve.cid, P, Q))
    assert ol.limbs_to_ints(got) == pool.product(range(n))
    assert got.tobytes() == _with_env({}, lambda: backend.pairing_product(curve.cid, P, Q)).tobytes()
    if n <= 64:
        assert (got == hook_pairing_product(curve.cid, P, Q)).all()


# ---- b. ones inside shared groups ----------------------------------------------------------------------------------------------------------------------
def test_ones_inside_shared_groups(backend, pool):
    curve, n, t = pool.curve, 7, 3
    G, ng, npad = _geometry(n, t)
    assert (G, ng) == (3, 3) and npad == n + 2  # two padding lanes, both copies of pair 0
    run = lambda P, Q: ol.limbs_to_ints(_with_env(_env(groups=t), lambda: backend.pairing_product(curve.cid, P, Q)))
    # pair 0 at infinity: the padding lanes copy it, the other pairs are untouched
    P, Q = pool.P[:n].copy(), pool.Q[:n].copy()
    P[0] = 0
    assert run(P, Q) == pool.product(range(1, n))
    # a Q at infinity in the middle of a group: pair 3 is the second of the three pairs of group 0
    mid = 3
    assert mid % ng == 0 and mid // ng == 1 and mid + ng < n
    P, Q = pool.P[:n].copy(), pool.Q[:n].copy()
    Q[mid] = 0
    assert run(P, Q) == pool.product([i for i in range(n) if i != mid])
    # every pair at infinity, on either side
    P, Q = pool.P[:n].copy(), pool.Q[:n].copy()
    P[0::2] = 0
    Q[1::2] = 0
    assert run(P, Q) == ONE
    # e(a P, Q) e(P, -a Q) = 1: the two pairs in one group, then in two groups
    a, r = 0x5EED5EED5EED, curve.fr.p
    Pi = ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs([a, 1], 4))
    Qi = gu.g2_mul_gen(curve, [1, r - a])
    for i, j, same in ((1, 4, True), (1, 5, False)):
        assert (i % ng == j % ng) == same
        P, Q = pool.P[:n].copy(), pool.Q[:n].copy()
        P[i], Q[i], P[j], Q[j] = Pi[0], Qi[0], Pi[1], Qi[1]
        assert run(P, Q) == pool.product([k for k in range(n) if k not in (i, j)]), (i, j)


# ---- c. the level boundaries of k_pd_prod with a group per pair ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("n,levels", [(16, 1), (17, 2), (256, 2), (257, 3)])
def test_group_product_level_boundaries(backend, curve, n, levels):
    G, ng, npad = _geometry(n, 32 * _cu_count())
    assert (G, ng, npad) == (1, n, n) and _prod_levels(ng) == levels
    P, Q, exp = _bilinear(backend, curve, n, 41)
    assert (_with_env({}, lambda: backend.pairing_product(curve.cid, P, Q)) == exp).all()


# ---- d. several launch sets ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [None, 3], ids=["default_groups", "groups3"])
@pytest.mark.parametrize("n,pair_set", [(3, 1), (21, 8), (21, 20), (21, 21)], ids=lambda v: str(v))
def test_launch_sets(backend, pool, n, pair_set, groups):
    sets = _sets(n, groups if groups else 32 * _cu_count(), pair_set)
    assert len(sets) == -(-n // pair_set) and sets[-1][0] + sets[-1][1] == n
    assert (len(sets) == 1) == (pair_set == n)
    if pair_set == 20:
        assert sets[-1][1] == 1  # a last set of one pair
    if groups and pair_set == 8:
        assert sets[0][2] == 3 and sets[-1][2] == 2 and all(s[4] > s[1] for s in sets)  # the last set has another G; every set pads
    if groups is None:
        assert all(s[2] == 1 for s in sets)
    curve, P, Q = pool.curve, pool.P[:n], pool.Q[:n]
    got = _with_env(_env(groups=groups, pair_set=pair_set), lambda: backend.pairing_product(curve.cid, P, Q))
    assert ol.limbs_to_ints(got) == pool.product(range(n))
    assert got.tobytes() == _with_env({}, lambda: backend.pairing_product(curve.cid, P, Q)).tobytes()
    assert (got == hook_pairing_product(curve.cid, P, Q)).all()


def test_pair_set_is_clamped(backend, pool):
    """values below 1 are one pair per set, values above MAX_PAIRS are MAX_PAIRS; ZL_TUNE_PAIR_GROUPS below 1 is the default"""
    curve, P, Q = pool.curve, pool.P[:5], pool.Q[:5]
    exp = pool.product(range(5))
    for knobs in (_env(pair_set=0), _env(pair_set=-3), _env(pair_set=MAX_PAIRS * 4), _env(groups=0), _env(groups=-1)):
        assert ol.limbs_to_ints(_with_env(knobs, lambda: backend.pairing_product(curve.cid, P, Q))) == exp, knobs


# ---- e. the 128-bit scalars of the batch verifier ------------------------------------------------------------------------------------------------------
SCALED_N = 22
INF_AT = 9  # a P at infinity under a non-zero scalar
SCALED_GEOMETRIES = [(None, None), (3, None), (None, 4), (3, 4), (3, 7)]


def _scalars():
    rng = np.random.Generator(np.random.PCG64(0x5CA1AB1E))
    fixed = [(1 << 64) - 1, 0, 1, 2, 1 << 64, 1 << 127, (1 << 128) - 1]
    ks = fixed + [int(lo) | (int(hi) << 64) for lo, hi in rng.integers(0, 1 << 64, size=(SCALED_N - len(fixed), 2), dtype=np.uint64)]
    assert len(set(ks)) == SCALED_N and ks[0] != 1 and ks[INF_AT] != 0
    return ks


@pytest.mark.parametrize("groups,pair_set", SCALED_GEOMETRIES, ids=lambda v: str(v))
def test_scaled_products(backend, pool, groups, pair_set):
    curve, n, r = pool.curve, SCALED_N, pool.curve.fr.p
    sets = _sets(n, groups if groups else 32 * _cu_count(), pair_set if pair_set else MAX_PAIRS)
    if groups and not pair_set:
        assert len(sets) == 1 and sets[0][2] > 1 and sets[0][4] > n  # padding lanes read pair 0, whose scalar is not 1
    if pair_set:
        assert len(sets) > 1 and sets[1][0] == pair_set  # the scalars of a later set start at 4 * first words
    if (groups, pair_set) == (3, 7):
        assert all(s[4] > s[1] for s in sets[:-1]) and sets[1][2] > 1  # later sets share groups and pad, with their own pair 0
    ks = _scalars()
    P, Q = pool.P[:n].copy(), pool.Q[:n].copy()
    P[INF_AT] = 0
    k128 = ol.ints_to_limbs(ks, 2)
    # the expected points (k_i a_i mod r) G1 from the oracle; a zero scalar and the point at infinity are all-zero records
    kP = ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs([k * a % r for k, a in zip(ks, pool.a[:n])], 4))
    for i in range(n):
        if ks[i] * pool.a[i] % r == 0 or i == INF_AT:
            kP[i] = 0
    assert not kP[1].any() and not kP[INF_AT].any() and sum(1 for i in range(n) if not kP[i].any()) == 2
    exp = hook_pairing_product(curve.cid, kP, Q)
    got = _with_env(_env(groups=groups, pair_set=pair_set), lambda: hook_pairing_product_scaled(backend, curve.cid, P, Q, k128))
    assert (got == exp).all()
    # no scalars: the unscaled product of the same geometry
    plain = _with_env(_env(groups=groups, pair_set=pair_set), lambda: hook_pairing_product_scaled(backend, curve.cid, P, Q, None))
    assert plain.tobytes() == _with_env({}, lambda: backend.pairing_product(curve.cid, P, Q)).tobytes()
    assert ol.limbs_to_ints(plain) == pool.product([i for i in range(n) if i != INF_AT])


def test_a_zero_scalar_contributes_one(backend, pool):
    curve = pool.curve
    zero = np.zeros((1, 2), dtype=np.uint64)
    assert ol.limbs_to_ints(hook_pairing_product_scaled(backend, curve.cid, pool.P[:1], pool.Q[:1], zero)) == ONE
    # as pair 0 of a padded launch, whose padding lanes read that scalar too
    k128 = ol.ints_to_limbs([0, 1, 1], 2)
    assert _geometry(3, 2) == (2, 2, 4)
    got = _with_env(_env(groups=2), lambda: hook_pairing_product_scaled(backend, curve.cid, pool.P[:3], pool.Q[:3], k128))
    assert ol.limbs_to_ints(got) == pool.product([1, 2])


# ---- f. the batch verifier under these geometries ------------------------------------------------------------------------------------------------------
NPROOFS = 8


@pytest.fixture(scope="module", params=CURVES, ids=lambda c: c.name)
def poseidon(request, backend):
    """eight 235-constraint Poseidon proofs over one key, each of another witness and so of another public input, and the key's verifying key as points"""
    curve = request.param
    circ = Circuit(curve.cid, 1)
    keys = Groth16Keys(backend, circ, seed=0x6E0)
    wits = [Circuit(curve.cid, 1, x0=3 + 2 * j, x1=1000 + 7 * j, witness_only=True) for j in range(NPROOFS)]
    proofs = keys.prove_many(list(range(700, 700 + NPROOFS)), circuits=wits)
    pubs = np.stack([w.arrays()["assignment"][1:2] for w in wits])
    for w in wits:
        w.close()
    assert pubs.shape == (NPROOFS, 1, 4) and len({p.tobytes() for p in pubs}) == NPROOFS
    al, be, ga, de, tau = keys.trapdoor()
    ex = po.groth16_setup_exponents(curve, po.poseidon_chain_circuit(curve.fr, 1), po.Groth16Trapdoor(alpha=al, beta=be, gamma=ga, delta=de, tau=tau))
    vk = {"alpha_g1": ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs([al], 4))[0], "beta_g2": gu.g2_mul_gen(curve, [be])[0],
          "gamma_g2": gu.g2_mul_gen(curve, [ga])[0], "delta_g2": gu.g2_mul_gen(curve, [de])[0],
          "gamma_abc": ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs(ex["gamma_abc"], 4))}
    yield curve, keys, proofs, pubs, vk
    keys.close()
    circ.close()


@pytest.mark.parametrize("groups,pair_set", [(3, None), (None, 4), (3, 4)], ids=lambda v: str(v))
def test_accepted_batch_under_small_geometries(poseidon, groups, pair_set):
    curve, keys, proofs, pubs, vk = poseidon
    npairs = NPROOFS + 3
    sets = _sets(npairs, groups if groups else 32 * _cu_count(), pair_set if pair_set else MAX_PAIRS)
    if pair_set:
        assert len(sets) == 3
    if groups and not pair_set:
        assert sets[0][2:] == (4, 3, 12)  # shared groups, one padding lane, scalars
    hok, heach = hook_verify_batch_host(curve.cid, vk, proofs, pubs, 1, seed=5)
    assert hok is True and heach.all()
    ok, each = _with_env(_env(groups=groups, pair_set=pair_set), lambda: keys.verify_batch(proofs, pubs, seed=5, each=True))
    assert ok is True and each.tobytes() == heach.tobytes()


REJECTS = [
    {1: "other_a"},  # the first reject-path set
    {3: "public"},  # a middle set
    {4: "wrong_c"},
    {7: "public"},  # the last set
    {0: "a_inf", 2: "public", 5: "other_a", 7: "wrong_c"},  # one in every set
]


@pytest.mark.parametrize("dev_min", [1, HOST_ONLY], ids=["device_fexp", "host_fexp"])
@pytest.mark.parametrize("plan", REJECTS, ids=lambda p: "+".join(f"{i}{k}" for i, k in p.items()))
def test_rejected_batch_in_sets_of_two_proofs(poseidon, plan, dev_min):
    curve, keys, proofs, pubs, vk = poseidon
    pair_set = 8
    per = max(1, pair_set // 4)
    firsts = list(range(0, NPROOFS, per))
    assert firsts == [0, 2, 4, 6]
    if len(plan) > 1:
        assert {i // per for i in plan} == {0, 1, 2, 3}
    bad, bpubs = _tamper(proofs, pubs, plan)
    expected = [i not in plan for i in range(NPROOFS)]
    hok, heach = hook_verify_batch_host(curve.cid, vk, bad, bpubs, 1, seed=13)
    assert hok is False and [bool(e) for e in heach] == expected
    ok, each = _with_env(_env(pair_set=pair_set, dev_min=dev_min), lambda: keys.verify_batch(bad, bpubs, seed=13, each=True))
    assert ok is False
    assert each.tobytes() == heach.tobytes()


# ---- g. the default geometry, no knob ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_default_geometry_product_shares_groups_and_pads(backend, curve):
    target = 32 * _cu_count()
    n = target + 1
    G, ng, npad = _geometry(n, target)
    assert G == 2 and npad == n + 1
    P, Q, exp = _bilinear(backend, curve, n, 51)
    assert (_with_env({}, lambda: backend.pairing_product(curve.cid, P, Q)) == exp).all()


def test_default_geometry_batch_shares_groups_and_pads(poseidon):
    curve, keys, proofs, pubs, vk = poseidon
    target = 32 * _cu_count()
    count = target - 2
    G, ng, npad = _geometry(count + 3, target)
    assert G == 2 and npad == count + 4
    idx = np.arange(count) % NPROOFS
    tiled, tpubs = [proofs[i] for i in idx], np.ascontiguousarray(pubs[idx])
    assert _with_env({}, lambda: keys.verify_batch(tiled, tpubs, seed=29)) is True
    wrong = tpubs.copy()
    wrong[count - 5, 0, 0] ^= np.uint64(1)
    assert _with_env({}, lambda: keys.verify_batch(tiled, wrong, seed=29, each=False)) is False
