"""Groth16 proving over keys whose queries carry window tables (zl_bases_precompute), at shapes of a few hundred points.  The headline proof runs all five of
its MSMs over such handles, but Groth16::build_window_tables makes them only for queries of 2^19 points and more, so every other proof test runs on plain
handles.  Here the tables are built on small keys -- by zl_bases_precompute on raw handles, and by compile / decode with ZL_TUNE_G16_TABLE_MIN_LOG = 1 -- and
every prover that reads those handles runs over them.

Expected values: the CPU oracle's proof (groth16_util.oracle_prove) and, where the prover leaves it, the quotient h (groth16_last_h); for the provers of
compiled keys (lanes, the two-lane stream, the batch and chain provers) the proof of the same key without tables, byte for byte.  Every case first asserts
through hook_msm_plan, on the (first, n) ranges the prover's jobs use, that the plan is the table plan (pre == 1) of the expected width: a table that is
silently ignored fails the case instead of emptying it.

  (a) raw handles longer than the jobs, all five with tables: folded / four-MSM C, side by side / pipeline, canonical / Montgomery   -> test_raw_key_*
  (b) tables on some of the queries only                                                                                          -> test_mixed_key_on_the_pipeline
  (c) 0/1-heavy and edge assignments: the scalar-1 bypass and a giant bucket at first = 1 on a table                               -> test_edge_assignments_on_table_handles
  (d) tables added and rebuilt under a live key cache                                                                              -> test_table_lifecycle_under_a_live_key_cache
  (e) compiled and decoded keys through ZL_TUNE_G16_TABLE_MIN_LOG                                                                  -> test_compiled_*
  (f) one proof over three virtual ranks, a table per shard                                                                        -> test_sharded_table_per_shard
  (g) a table is refused while a caller's fork lives                                                                               -> test_precompute_refused_beside_a_fork

The job ranges (csrc/zl_groth16.hip): a, b1 and b2 take points [1, nv) with the scalars z[1:], l takes [0, nw) with z[ni:], h takes [0, N - 1)."""
import collections
import contextlib
import itertools
import os

import numpy as np
import pytest

import groth16_util as gu
import oracle_lib as ol
import r1cs_gen as rg
from oracle_lib import po
from openzl_amd import ZL_G1, ZL_G2, ZL_MONT, BackendError, Circuit, Groth16Keys, MultiBackend, poseidon_chain_assignments_host
from openzl_amd.backend import hook_msm_plan

pytestmark = pytest.mark.gpu

CURVES = [po.BLS12_381, po.BN254]
CURVE = pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
QUERIES = ("a_query", "b_g1_query", "h_query", "l_query", "b_g2_query")
ALL16 = {q: 16 for q in QUERIES}
DEFAULT_C = {q: (16 if q == "b_g2_query" else 20) for q in QUERIES}  # build_window_tables: G1 20, G2 16
KEY_NV, KEY_NW, KEY_NH = 700, 700, 600  # longer than every job of the shapes below (nv <= 302, N - 1 <= 511)
EINVAL = -1
FOLD, SIDE = "ZL_TUNE_G16_FOLD_LOG_N", "ZL_TUNE_SIDE_BY_SIDE_LOG"
KNOBS = (FOLD, SIDE, "ZL_TUNE_G16_TABLE_MIN_LOG", "ZL_TUNE_G1_TABLE_C", "ZL_TUNE_G2_TABLE_C", "ZL_TUNE_G16_BATCH_LOG_N", "ZL_TUNE_G16_BATCH_MIN",
         "ZL_TUNE_G16_BATCH_CHUNK", "ZL_TUNE_SPMV8", "ZL_TUNE_NTT_BATCH_LOG_N")


@contextlib.contextmanager
def _env(**kv):
    """the environment with every knob of this file unset but those given, put back on exit"""
    old = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        for k, v in kv.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(autouse=True)
def _knobs_unset():
    with _env():
        yield


def _same(got, exp):
    for g, e in zip(got, exp):
        assert np.array_equal(np.asarray(g), np.asarray(e))


def _is_same(p, q):
    return all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(p, q))


def _to_mont(curve, z):
    zm = np.zeros_like(z)
    fid = 2 if curve.cid == 1 else 4  # the oracle's Fr ids
    assert ol.lib().zlo_field_to_mont(fid, ol.p64(np.ascontiguousarray(z).reshape(-1)), ol.p64(zm.reshape(-1)), z.shape[0]) == 0
    return zm


def _job_ranges(nv: int, ni: int, n_domain: int) -> dict:
    """query -> (first, n) of the prover's job over it"""
    return {"a_query": (1, nv - 1), "b_g1_query": (1, nv - 1), "b_g2_query": (1, nv - 1), "l_query": (0, nv - ni), "h_query": (0, n_domain - 1)}


def _assert_plans(backend, dpk: dict, ranges: dict, widths: dict):
    """the plan of every job: the table plan of width widths[query], or no table for a query that widths does not name"""
    for q, (first, n) in ranges.items():
        plan = hook_msm_plan(backend, dpk[q], n, first)
        if q in widths:
            assert plan.pre == 1 and plan.c == widths[q] and plan.SETS == 1 and plan.wide == 1 and plan.glv == 0, (q, plan)
        else:
            assert plan.pre == 0, (q, plan)


def _precompute(backend, dpk: dict, widths: dict):
    for q, c in widths.items():
        backend.bases_precompute(dpk[q], c)


# ---- raw-handle keys: random points with known discrete logs, the same points under every device key of a curve --------------------------------------
_SEED = 0x7AB1E
SINGLES = ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2")
# one proof to make: the circuit's arrays, the assignment, the blinding scalars, the domain size N, query -> (first, n) of the prover's jobs, and the oracle's proof and h
Case = collections.namedtuple("Case", "arrays z r s n ranges proof h")


def _generate_queries(backend, curve) -> dict:
    """the five queries as device handles: the same points at every call (the scalars follow from the seed)"""
    return {name: backend.bases_generate(curve.cid, ol.random_scalars(curve, n, _SEED + 16 * curve.cid + i), group=group)
            for i, (name, n, group) in enumerate((("a_query", KEY_NV, ZL_G1), ("b_g1_query", KEY_NV, ZL_G1), ("h_query", KEY_NH, ZL_G1), ("l_query", KEY_NW, ZL_G1),
                                                  ("b_g2_query", KEY_NV, ZL_G2)))}


@pytest.fixture(scope="module")
def hostkey(backend):
    """per curve: the raw key's points in host memory, for the oracle -- generated on the device, downloaded once, the handles freed"""
    made = {}

    def get(curve) -> dict:
        if curve.cid not in made:
            single = ol.limbs_to_ints(ol.random_scalars(curve, 5, _SEED + 16 * curve.cid + 7))
            g1 = ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs(single[:3], 4))
            g2 = gu.g2_mul_gen(curve, single[3:])
            handles = _generate_queries(backend, curve)
            try:
                hpk = {q: backend.bases_download(handles[q]) for q in QUERIES}
            finally:
                gu.free_pk(backend, handles)
            hpk.update(zip(SINGLES, (g1[0], g1[1], g1[2], g2[0], g2[1])))
            made[curve.cid] = hpk
        return made[curve.cid]

    return get


def _device_key(backend, curve, hpk: dict) -> dict:
    """a device key of its own over the points of hpk"""
    dpk = _generate_queries(backend, curve)
    dpk.update({k: hpk[k] for k in SINGLES})
    return dpk


@contextlib.contextmanager
def _fresh_key(backend, curve, hpk: dict):
    dpk = _device_key(backend, curve, hpk)
    try:
        yield dpk
    finally:
        gu.free_pk(backend, dpk)


@pytest.fixture(scope="module")
def raw(backend, hostkey):
    """per curve: one device key with a table of width 16 on all five queries, shared by the cases that do not change tables"""
    made = {}

    def get(curve) -> dict:
        if curve.cid not in made:
            made[curve.cid] = _device_key(backend, curve, hostkey(curve))
            _precompute(backend, made[curve.cid], ALL16)
        return made[curve.cid]

    yield get
    for dpk in made.values():
        gu.free_pk(backend, dpk)


def _assignment(curve, cs, variant: str) -> list:
    """variant: "own" = the circuit's assignment; (c)'s names = its witness part overwritten"""
    ni, nw, p = cs.n_instance, cs.n_witness, curve.fr.p
    zi = cs.assignment()
    if variant == "own":
        return zi
    if variant == "ones":
        return zi[:ni] + [1] * nw
    if variant == "zeros":
        return zi[:ni] + [0] * nw
    if variant == "r_minus_1":
        return zi[:ni] + [p - 1] * nw
    assert variant == "mostly_01"  # 60 % zeros, 30 % ones, the rest uniform
    u = np.random.Generator(np.random.PCG64(61)).random(nw)
    rnd = ol.limbs_to_ints(ol.random_scalars(curve, nw, 62))
    return zi[:ni] + [0 if x < 0.6 else (1 if x < 0.9 else v) for x, v in zip(u, rnd)]


@pytest.fixture(scope="module")
def cases(hostkey):
    """(curve, shape of r1cs_gen.SHAPES, variant) -> Case over the raw key, the oracle's proof and h computed once and shared"""
    made = {}

    def get(curve, name: str, variant: str = "own") -> Case:
        key = (curve.cid, name, variant)
        if key not in made:
            cs, arrays = rg.shape_case(curve, name)
            n = 1 << cs.domain_log()
            z = ol.ints_to_limbs(_assignment(curve, cs, variant), 4)
            r, s = ol.random_scalars(curve, 2, 0x515 + len(name))
            proof, h = gu.oracle_prove(curve, arrays, z, hostkey(curve), r, s, threads=8, want_h=n)
            made[key] = Case(arrays, z, r, s, n, _job_ranges(cs.n_instance + cs.n_witness, cs.n_instance, n), proof, h)
        return made[key]

    return get


def _prove_checked(backend, curve, dpk, case: Case, what):
    got = backend.groth16_prove(curve.cid, dpk, case.arrays, case.z, case.r, case.s)
    assert (backend.groth16_last_h(case.n) == case.h).all(), what
    _same(got, case.proof)
    return got


def _resident_checked(be, curve, dpk, hr, case: Case, what, z=None, flags=0):
    got = be.groth16_prove_resident(curve.cid, dpk, hr, case.z if z is None else z, case.r, case.s, flags=flags)
    assert (be.groth16_last_h(case.n) == case.h).all(), what
    _same(got, case.proof)
    return got


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse_a", "mixed", "many_publics"])
@CURVE
def test_raw_key_every_form_matches_oracle(backend, raw, cases, curve, name):
    """all five handles with tables, each longer than its job (h is a sub-range of its table, a / b1 / b2 start at point 1): zl_groth16_prove, and
    zl_groth16_prove_resident from canonical and Montgomery limbs, with C folded (job 0 on a table handle, job 1 on the query concatenated from table handles)
    or from four MSMs, the G1 jobs side by side or on the three-stream pipeline: proof and h equal the oracle's in every setting"""
    dpk = raw(curve)
    case = cases(curve, name)
    _assert_plans(backend, dpk, case.ranges, ALL16)
    zm = _to_mont(curve, case.z)
    hr = backend.r1cs_upload(curve.cid, case.arrays)
    try:
        for fold, side in itertools.product(("0", "20"), (None, "0")):
            with _env(**{FOLD: fold, **({SIDE: side} if side is not None else {})}):
                _prove_checked(backend, curve, dpk, case, (fold, side))
                _resident_checked(backend, curve, dpk, hr, case, (fold, side, "canonical"))
                _resident_checked(backend, curve, dpk, hr, case, (fold, side, "Montgomery"), z=zm, flags=ZL_MONT)
    finally:
        backend.r1cs_free(hr)


@CURVE
def test_raw_key_default_widths(backend, hostkey, cases, curve):
    """the widths build_window_tables gives a large key (G1 20: 2^19 buckets, G2 16), both forms of C; one shape per curve (0.07 s BLS12-381, 0.04 s BN254
    on the MI355X for the two proofs: the wider bucket set does not show at this size)"""
    case = cases(curve, "sparse_a")
    with _fresh_key(backend, curve, hostkey(curve)) as dpk:
        _precompute(backend, dpk, DEFAULT_C)
        _assert_plans(backend, dpk, case.ranges, DEFAULT_C)
        for fold in ("0", "20"):
            with _env(**{FOLD: fold}):
                _prove_checked(backend, curve, dpk, case, fold)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse_a", "mixed"])
@pytest.mark.parametrize("tabled", [("a_query", "b_g2_query"), ("h_query", "l_query"), ("b_g1_query",)], ids="+".join)
@CURVE
def test_mixed_key_on_the_pipeline(backend, hostkey, cases, curve, tabled, name):
    """what a key with nw < 2^19 <= nv gets: tables on some queries only, so the four G1 jobs of one pipeline differ in plan, n and handle while the G2
    job (with or without a table) runs on its worker"""
    case = cases(curve, name)
    widths = {q: 16 for q in tabled}
    with _fresh_key(backend, curve, hostkey(curve)) as dpk:
        _precompute(backend, dpk, widths)
        _assert_plans(backend, dpk, case.ranges, widths)
        hr = backend.r1cs_upload(curve.cid, case.arrays)
        try:
            with _env(**{FOLD: "0", SIDE: "0"}):
                _prove_checked(backend, curve, dpk, case, tabled)
                _resident_checked(backend, curve, dpk, hr, case, tabled)
        finally:
            backend.r1cs_free(hr)


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["ones", "zeros", "r_minus_1", "mostly_01"])
@CURVE
def test_edge_assignments_on_table_handles(backend, raw, cases, curve, variant):
    """sparse_a with its witness part overwritten (unsatisfied, which the prover accepts): every scalar 1 (the bypass takes the whole range, from point
    first = 1 of the table's base row), every scalar 0, every scalar r - 1 (one giant bucket per window), and a 0/1-heavy mix -- for the G1 jobs and the G2 job"""
    dpk = raw(curve)
    case = cases(curve, "sparse_a", variant)
    _assert_plans(backend, dpk, case.ranges, ALL16)
    for fold, side in (("0", None), ("20", None), ("0", "0")):
        with _env(**{FOLD: fold, **({SIDE: side} if side is not None else {})}):
            _prove_checked(backend, curve, dpk, case, (variant, fold, side))


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------------------------
@CURVE
def test_table_lifecycle_under_a_live_key_cache(backend, hostkey, cases, curve):
    """the key cache (fixed-base tables, folded query) is keyed by handle values, which a table does not change: plain, then tables of width 16, then
    rebuilt at 17, then twice more, alternating folded and four-MSM C -- one proof throughout"""
    case = cases(curve, "sparse_a")
    ranges = case.ranges
    all17 = {q: 17 for q in QUERIES}
    with _fresh_key(backend, curve, hostkey(curve)) as dpk:
        proofs = []
        steps = (("20", None), ("0", ALL16), ("20", all17), ("0", None), ("20", None))
        widths = {}
        for fold, build in steps:
            if build is not None:
                _precompute(backend, dpk, build)
                widths = build
            _assert_plans(backend, dpk, ranges, widths)
            with _env(**{FOLD: fold}):
                proofs.append(_prove_checked(backend, curve, dpk, case, (fold, widths)))
        assert widths == all17
        assert all(_is_same(p, proofs[0]) for p in proofs[1:])


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------------------------
def _chain_ranges(circ) -> dict:
    nc, ni, nw = circ.shape
    return _job_ranges(ni + nw, ni, 1 << max(1, (nc + ni - 1).bit_length()))


@pytest.fixture(scope="module")
def compiled(backend):
    """per curve, for the one-hash Poseidon circuit (237 variables beside ONE, N = 256): keys compiled with no knob set, keys of the same seed compiled with
    ZL_TUNE_G16_TABLE_MIN_LOG = 1 and both table widths 16, and those keys' bytes decoded under the same knobs"""
    made = {}

    def get(curve):
        if curve.cid not in made:
            full = Circuit(curve.cid, 1)
            with _env():
                plain = Groth16Keys(backend, full, seed=77)
            with _env(ZL_TUNE_G16_TABLE_MIN_LOG=1, ZL_TUNE_G1_TABLE_C=16, ZL_TUNE_G2_TABLE_C=16):
                table = Groth16Keys(backend, full, seed=77)
                decoded = Groth16Keys.from_bytes(backend, full, table.to_bytes())
            ranges = _chain_ranges(full)
            _assert_plans(backend, plain.pk_dict(), ranges, {})
            for keys in (table, decoded):
                _assert_plans(backend, keys.pk_dict(), ranges, ALL16)
                assert _is_same(keys.prove(seed=5)[0], plain.prove(seed=5)[0])  # (a decoded key binds its circuit on its first proof, on its own ctx)
            made[curve.cid] = dict(full=full, plain=plain, compiled=table, decoded=decoded, ranges=ranges)
        return made[curve.cid]

    yield get
    for m in made.values():
        for k in ("plain", "compiled", "decoded"):
            m[k].close()
        m["full"].close()


KIND = pytest.mark.parametrize("kind", ["compiled", "decoded"])


@CURVE
def test_compiled_keys_carry_tables_only_through_the_knob(backend, curve):
    """ZL_TUNE_G16_TABLE_MIN_LOG = 1: compile and decode build all five tables, of the default widths and of the widths ZL_TUNE_G1_TABLE_C / ZL_TUNE_G2_TABLE_C
    name; unset (and 0): a key of the same seed has none.  One proof over the default-width key equals the oracle's and verifies; a flipped public input
    is rejected."""
    full = Circuit(curve.cid, 1)
    ranges = _chain_ranges(full)
    made = []

    def keys_under(**env):
        with _env(**env):
            k = Groth16Keys(backend, full, seed=78)
            made.append(k)
            d = Groth16Keys.from_bytes(backend, full, k.to_bytes())
            made.append(d)
        return k, d

    try:
        for k in keys_under():
            _assert_plans(backend, k.pk_dict(), ranges, {})
        for k in keys_under(ZL_TUNE_G16_TABLE_MIN_LOG=0):
            _assert_plans(backend, k.pk_dict(), ranges, {})
        for k in keys_under(ZL_TUNE_G16_TABLE_MIN_LOG=1, ZL_TUNE_G1_TABLE_C=16, ZL_TUNE_G2_TABLE_C=17):
            _assert_plans(backend, k.pk_dict(), ranges, {q: (17 if q == "b_g2_query" else 16) for q in QUERIES})
        plain = made[0]
        for k in keys_under(ZL_TUNE_G16_TABLE_MIN_LOG=1):
            pk = k.pk_dict()
            _assert_plans(backend, pk, ranges, DEFAULT_C)
            proof, r, s = k.prove(seed=9)
            arrays = full.arrays()
            hpk = dict(pk, **{q: backend.bases_download(pk[q]) for q in QUERIES})
            exp, _ = gu.oracle_prove(curve, arrays, arrays["assignment"], hpk, r, s, threads=8)
            _same(proof, exp)
            assert _is_same(proof, plain.prove(seed=9)[0])
            pub = arrays["assignment"][1:full.shape[1]]
            assert k.verify(proof, pub)
            flipped = pub.copy()
            flipped[0, 0] ^= np.uint64(1)
            assert not k.verify(proof, flipped)
    finally:
        for k in made:
            k.close()
        full.close()


@KIND
@CURVE
def test_compiled_prove_lane_and_stream(backend, compiled, curve, kind):
    """Groth16::prove on the keys' ctx and on a forked lane, and zl_groth16_prove_circuits over three circuits on its two lanes: the plain key's proofs"""
    m = compiled(curve)
    keys, plain = m[kind], m["plain"]
    _assert_plans(backend, keys.pk_dict(), m["ranges"], ALL16)
    wits = [Circuit(curve.cid, 1, x0=10 + j, x1=3 * j, witness_only=True) for j in range(2)]
    circs = [m["full"]] + wits
    seeds = [300, 301, 302]
    lane = backend.fork()
    try:
        ref = [plain.prove(seed=sd, circuit=c)[0] for sd, c in zip(seeds, circs)]
        for sd, c, e in zip(seeds, circs, ref):
            assert _is_same(keys.prove(seed=sd, circuit=c)[0], e)
            assert _is_same(keys.prove(seed=sd, circuit=c, lane=lane)[0], e)
    finally:
        lane.close()
    try:
        many = keys.prove_many(seeds, circs)  # (the lane the library keeps afterwards is idle and pins nothing: the next entry that minds releases it)
        assert len(many) == 3 and all(_is_same(a, b) for a, b in zip(many, ref))
        assert keys.verify(many[1], wits[0].arrays()["assignment"][1:2])
    finally:
        for c in wits:
            c.close()


def _chain_inputs(curve, count):
    x0 = ol.ints_to_limbs([3 + 2 * j for j in range(count)], 4)
    x1 = ol.ints_to_limbs([1000 + 7 * j for j in range(count)], 4)
    rs = ol.random_scalars(curve, 2 * count, 0xBA7C + count)
    return x0, x1, np.ascontiguousarray(rs[:count]), np.ascontiguousarray(rs[count:])


@pytest.mark.parametrize("count", [1, 2, 70])
@KIND
@CURVE
def test_compiled_prove_batch_on_the_device_path(backend, compiled, curve, kind, count):
    """the batched prover builds its extended queries from the table handles for zl_msm_multi_dev, which ignores tables: the plain key's proofs, which are the
    resident prover's over the table key; 70 assignments in two chunks"""
    m = compiled(curve)
    keys, plain = m[kind], m["plain"]
    _assert_plans(backend, keys.pk_dict(), m["ranges"], ALL16)
    x0, x1, r, s = _chain_inputs(curve, count)
    Z = poseidon_chain_assignments_host(curve.cid, x0, x1, 1)
    assert len({Z[j].tobytes() for j in range(count)}) == count
    with _env(ZL_TUNE_G16_BATCH_LOG_N=28, ZL_TUNE_G16_BATCH_MIN=1, **({"ZL_TUNE_G16_BATCH_CHUNK": 35} if count == 70 else {})):
        got = keys.prove_batch(Z, r, s)
        with pytest.raises(BackendError) as e:
            backend.groth16_last_h(2)  # the device path ran: no single quotient
        assert e.value.code == EINVAL
        ref = plain.prove_batch(Z, r, s)
    assert len(got) == count and all(_is_same(a, b) for a, b in zip(got, ref))
    hr = backend.r1cs_upload(curve.cid, m["full"].arrays())
    try:
        for j in {0, count - 1}:
            assert _is_same(got[j], backend.groth16_prove_resident(curve.cid, keys.pk_dict(), hr, Z[j], r[j], s[j]))
    finally:
        backend.r1cs_free(hr)
    assert keys.verify_batch(got, Z[:, 1:m["full"].shape[1]])


@KIND
@CURVE
def test_compiled_prove_chains(backend, compiled, curve, kind):
    """chain inputs in, proofs out, over a key with tables: the plain key's proofs and public inputs"""
    m = compiled(curve)
    keys, plain = m[kind], m["plain"]
    _assert_plans(backend, keys.pk_dict(), m["ranges"], ALL16)
    x0, x1, r, s = _chain_inputs(curve, 5)
    with _env(ZL_TUNE_G16_BATCH_LOG_N=28, ZL_TUNE_G16_BATCH_MIN=1):
        got, pub = keys.prove_chains(x0, x1, r, s)
        ref, ref_pub = plain.prove_chains(x0, x1, r, s)
    assert len(got) == 5 and all(_is_same(a, b) for a, b in zip(got, ref)) and (pub == ref_pub).all()
    assert keys.verify_batch(got, pub.reshape(5, 1, 4))


# ---- (f) ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse_a", "mixed", "many_publics"])
@CURVE
def test_sharded_table_per_shard(backend, raw, hostkey, cases, curve, name):
    """three virtual ranks, every rank's five slices with a table built on that rank's ctx (many_publics: l slices of 2, 2 and 3 points): the oracle's
    proof, which is the unsharded table key's, and the oracle's h, which the sharded prover leaves on rank 0"""
    dpk, hpk = raw(curve), hostkey(curve)
    case = cases(curve, name)
    single = _prove_checked(backend, curve, dpk, case, "unsharded")
    ni, nw, n = case.arrays["n_instance"], case.arrays["n_witness"], case.n
    pk = dict(hpk, a_query=hpk["a_query"][: ni + nw], b_g1_query=hpk["b_g1_query"][: ni + nw], b_g2_query=hpk["b_g2_query"][: ni + nw],
              l_query=hpk["l_query"][:nw], h_query=hpk["h_query"][: n - 1])  # the shards tile exactly the ranges of the proof
    mb = MultiBackend([0, 0, 0])
    try:
        keys = mb.groth16_shard_keys(curve.cid, pk, case.arrays)
        try:
            for g in range(mb.size):
                handles = keys.rank_handles(g)
                assert set(handles) == set(QUERIES)
                for q, (hnd, cnt) in handles.items():
                    mb.ranks[g].bases_precompute(hnd, 16)
                    plan = hook_msm_plan(mb.ranks[g], hnd, cnt, 0)
                    assert plan.pre == 1 and plan.c == 16, (g, q, plan)
            got = keys.prove(case.z, case.r, case.s)
            h_got = mb.ranks[0].groth16_last_h(n)
            got_m = keys.prove(_to_mont(curve, case.z), case.r, case.s, mont=True)
            h_got_m = mb.ranks[0].groth16_last_h(n)
        finally:
            keys.close()
    finally:
        mb.close()
    assert (h_got == case.h).all() and (h_got_m == case.h).all()
    _same(got, case.proof)
    _same(got_m, case.proof)
    assert _is_same(got, single)


# ---- (g) ---------------------------------------------------------------------------------------------------------------------------------------------
@CURVE
def test_precompute_refused_beside_a_fork(backend, hostkey, cases, curve):
    """while a caller's fork lives, a table on a key's handle is refused (the lanes read what it would replace) and the key proves as before, on the ctx and
    on the lane; once the fork is closed the tables are built and the next proof is the same"""
    case = cases(curve, "many_publics")
    with _fresh_key(backend, curve, hostkey(curve)) as dpk:
        before = _prove_checked(backend, curve, dpk, case, "before")
        hr = backend.r1cs_upload(curve.cid, case.arrays)
        lane = backend.fork()
        try:
            for q in QUERIES:
                with pytest.raises(BackendError) as e:
                    backend.bases_precompute(dpk[q], 16)
                assert e.value.code == EINVAL
            _assert_plans(backend, dpk, case.ranges, {})
            _resident_checked(lane, curve, dpk, hr, case, "on the lane")
            _prove_checked(backend, curve, dpk, case, "beside the fork")
        finally:
            lane.close()
            backend.r1cs_free(hr)
        _precompute(backend, dpk, ALL16)
        _assert_plans(backend, dpk, case.ranges, ALL16)
        after = _prove_checked(backend, curve, dpk, case, "after")
        assert _is_same(before, after)
