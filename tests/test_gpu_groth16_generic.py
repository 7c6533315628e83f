"""Groth16 on the device for generic R1CS circuits (tests/r1cs_gen.py), bit-exact against the CPU oracle: proof bytes (a, b, c and the
three infinity flags) and the quotient h of the witness map, over the shape table of r1cs_gen.SHAPES on both curves, under every setting
of the knobs that pick the witness map's kernels (one- or eight-lane matrix-vector products, batched or single transforms) and the form
of C (folded query or four MSMs); then the resident matrices with canonical and Montgomery assignments, one key serving two circuit
shapes in turn, one proof over three virtual ranks, and a 2^19 domain with no knob set.  Parity cases use one key of random points per
curve (known discrete logs, not a setup of any circuit); the trapdoor cases also check the points the exponents predict."""
import itertools

import numpy as np
import pytest

import groth16_util as gu
import oracle_lib as ol
import r1cs_gen as rg
from oracle_lib import po
from openzl_amd import ZL_G1, ZL_G2, ZL_MONT, MultiBackend

pytestmark = pytest.mark.gpu

CURVES = [po.BLS12_381, po.BN254]
KNOBS = ("ZL_TUNE_SPMV8", "ZL_TUNE_G16_FOLD_LOG_N", "ZL_TUNE_NTT_BATCH_LOG_N")
TD = po.Groth16Trapdoor(alpha=0x5151_2323_7878, beta=0x2468_ACE0_1357, gamma=0x9BDF_1111, delta=0x7777_1234_4321, tau=0xABCD_EF01_2345_6789)


def _random_key(backend, curve, nv: int, nw: int, nh: int, seed: int):
    """(device pk, host pk): a key of random points made on the device (zl_bases_generate) and downloaded for the oracle"""
    dpk, hpk = {}, {}
    for i, (name, n, group) in enumerate((("a_query", nv, ZL_G1), ("b_g1_query", nv, ZL_G1), ("h_query", nh, ZL_G1), ("l_query", max(nw, 1), ZL_G1),
                                          ("b_g2_query", nv, ZL_G2))):
        dpk[name] = backend.bases_generate(curve.cid, ol.random_scalars(curve, n, seed + i), group=group)
        hpk[name] = backend.bases_download(dpk[name])
    single = ol.limbs_to_ints(ol.random_scalars(curve, 5, seed + 7))
    g1 = ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs(single[:3], 4))
    g2 = gu.g2_mul_gen(curve, single[3:])
    for k, v in zip(("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2"), (g1[0], g1[1], g1[2], g2[0], g2[1])):
        dpk[k] = hpk[k] = v
    return dpk, hpk


@pytest.fixture(scope="module")
def keys(backend):
    made = {}

    def get(curve):
        if curve.cid not in made:
            made[curve.cid] = _random_key(backend, curve, rg.KEY_NV, rg.KEY_NW, rg.KEY_NH, seed=0x6E6E + curve.cid)
        return made[curve.cid]

    yield get
    for dpk, _ in made.values():
        gu.free_pk(backend, dpk)


def _rs(curve, seed):
    r, s = ol.random_scalars(curve, 2, seed)
    return r, s


def _z(cs):
    return ol.ints_to_limbs(cs.assignment(), 4)


def _same(got, exp):
    for g, e in zip(got, exp):
        assert np.array_equal(np.asarray(g), np.asarray(e))


@pytest.mark.parametrize("name", list(rg.SHAPES))
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_gpu_generic_proof_matches_oracle(backend, keys, curve, name, monkeypatch):
    """every knob setting: ZL_TUNE_SPMV8 = 0 sends every matrix to the one-lane kernel, 1 the matrices of >= 4 terms per row to the eight-lane one;
    ZL_TUNE_G16_FOLD_LOG_N 0 / 20: four-MSM C / folded C; ZL_TUNE_NTT_BATCH_LOG_N 0 / 18: single / batched transforms"""
    cs, arrays = rg.shape_case(curve, name)
    n = 1 << cs.domain_log()
    dpk, hpk = keys(curve)
    z = _z(cs)
    r, s = _rs(curve, 11)
    exp, h = gu.oracle_prove(curve, arrays, z, hpk, r, s, threads=8, want_h=n)
    for setting in itertools.product(("0", "1"), ("0", "20"), ("0", "18")):
        for k, v in zip(KNOBS, setting):
            monkeypatch.setenv(k, v)
        got = backend.groth16_prove(curve.cid, dpk, arrays, z, r, s)
        assert (backend.groth16_last_h(n) == h).all(), setting
        _same(got, exp)


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_gpu_generic_trapdoor_proof_is_the_predicted_point(backend, curve):
    """smallest shape (N = 2) with a trapdoor key: the device proof is the group element the exponents give, and those satisfy the Groth16 equation"""
    cs, arrays = rg.shape_case(curve, "smallest")
    n = 1 << cs.domain_log()
    pk = gu.setup_with_trapdoor(curve, cs, TD)
    r, s = _rs(curve, 12)
    dpk = gu.upload_pk(backend, curve, pk)
    try:
        got = backend.groth16_prove(curve.cid, dpk, arrays, _z(cs), r, s)
        h_gpu = backend.groth16_last_h(n)
    finally:
        gu.free_pk(backend, dpk)
    exp, h = gu.oracle_prove(curve, arrays, _z(cs), pk, r, s, threads=8, want_h=n)
    assert (h_gpu == h).all()
    _same(got, exp)
    h_ints = ol.limbs_to_ints(h)
    A, B, Cx = po.groth16_prove_exponents(curve, cs, TD, pk["ex"], h_ints, *ol.limbs_to_ints(np.stack([r, s])))
    assert po.groth16_check_exponents(curve, cs, TD, pk["ex"], A, B, Cx)
    assert (got[0] == ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs([A], 4))[0]).all()
    assert (got[2] == gu.g2_mul_gen(curve, [B])[0]).all()
    assert (got[4] == ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs([Cx], 4))[0]).all()


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_gpu_generic_resident_matrices_canonical_and_montgomery(backend, keys, curve):
    """one upload of a generic CSR (zero / unsorted / repeated entries), three assignments -- satisfying, not satisfying, every witness r - 1 --
    each proved from canonical limbs and from Montgomery limbs (ZL_MONT): every proof and h equal the oracle's"""
    cs, arrays = rg.shape_case(curve, "edges")
    n = 1 << cs.domain_log()
    dpk, hpk = keys(curve)
    p = curve.fr.p
    ni, nw = cs.n_instance, cs.n_witness
    sat = cs.assignment()
    unsat = sat[:ni] + ol.limbs_to_ints(ol.random_scalars(curve, nw, 13))
    rmax = sat[:ni] + [p - 1] * nw
    fid = 2 if curve.cid == 1 else 4  # the oracle's Fr ids
    r, s = _rs(curve, 14)
    hr = backend.r1cs_upload(curve.cid, arrays)
    try:
        for i, zi in enumerate((sat, unsat, rmax)):
            z = ol.ints_to_limbs(zi, 4)
            zm = np.zeros_like(z)
            assert ol.lib().zlo_field_to_mont(fid, ol.p64(z.reshape(-1)), ol.p64(zm.reshape(-1)), z.shape[0]) == 0
            exp, h = gu.oracle_prove(curve, arrays, z, hpk, r, s, threads=8, want_h=n)
            assert (ol.limbs_to_ints(h)[-1] == 0) == (i == 0)
            for flags, zz in ((0, z), (ZL_MONT, zm)):
                got = backend.groth16_prove_resident(curve.cid, dpk, hr, zz, r, s, flags=flags)
                assert (backend.groth16_last_h(n) == h).all(), (i, flags)
                _same(got, exp)
    finally:
        backend.r1cs_free(hr)


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_gpu_generic_one_key_alternating_shapes(backend, keys, curve, monkeypatch):
    """one key's handles serve two circuits of different (n_variables, n_witness, N) in turn with the folded C query on: its cache drops and
    rebuilds the folded query at every switch, and every proof still equals the oracle's"""
    monkeypatch.setenv("ZL_TUNE_G16_FOLD_LOG_N", "20")
    dpk, hpk = keys(curve)
    cases = []
    for name in ("many_publics", "sparse_a"):
        cs, arrays = rg.shape_case(curve, name)
        n = 1 << cs.domain_log()
        r, s = _rs(curve, 15 + len(cases))
        exp, h = gu.oracle_prove(curve, arrays, _z(cs), hpk, r, s, threads=8, want_h=n)
        cases.append((arrays, _z(cs), r, s, n, exp, h))
    assert len({(c[0]["n_instance"] + c[0]["n_witness"], c[0]["n_witness"], c[4]) for c in cases}) == 2
    for arrays, z, r, s, n, exp, h in cases + cases:
        got = backend.groth16_prove(curve.cid, dpk, arrays, z, r, s)
        assert (backend.groth16_last_h(n) == h).all()
        _same(got, exp)


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_gpu_generic_sharded_over_virtual_ranks(keys, curve):
    """a generic circuit (five instance variables, empty C rows, few witnesses) through zl_groth16_prove_sharded over 3 virtual ranks"""
    cs = rg.generic_circuit(curve.fr, 16, 5, 14, mix={"boolean": 1, "empty": 1, "random": 1}, terms=(2, 2, 0), seed=31)
    arrays = gu.r1cs_arrays(cs)
    assert (np.diff(arrays["C"][0].astype(np.int64)) == 0).any()
    n = 1 << cs.domain_log()
    _, hpk = keys(curve)
    pk = dict(hpk, h_query=hpk["h_query"][: n - 1])  # the shards tile exactly N - 1 points of the h query
    r, s = _rs(curve, 17)
    exp, _ = gu.oracle_prove(curve, arrays, _z(cs), pk, r, s, threads=8, want_h=n)
    mb = MultiBackend([0, 0, 0])
    try:
        got = mb.groth16_prove_sharded(curve.cid, pk, arrays, _z(cs), r, s)
    finally:
        mb.close()
    _same(got, exp)


def test_gpu_generic_2p19_domain_bls(backend, monkeypatch):
    """n_constraints + n_instance = 2^18 + 1: N = 2^19, above the batched witness map (2^18) and the folded C (2^14) with no knob set;
    an unsatisfied assignment (full-degree h), rows of one to three terms over a small variable set"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    curve = po.BLS12_381
    ni, nw = 3, 61
    nc = (1 << 18) + 1 - ni
    nv = ni + nw
    rng = np.random.Generator(np.random.PCG64(19))
    arrays = {"n_constraints": nc, "n_instance": ni, "n_witness": nw}
    for m, key in enumerate("ABC"):
        lens = rng.integers(0 if key == "C" else 1, 4, size=nc)
        ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        col = rng.integers(0, nv, size=int(ptr[-1])).astype(np.uint32)
        val = ol.random_scalars(curve, int(ptr[-1]), 20 + m)
        arrays[key] = (ptr, col, val)
    z = np.concatenate([ol.ints_to_limbs([1], 4), ol.random_scalars(curve, nv - 1, 23)])
    n = 1 << 19
    dpk, hpk = _random_key(backend, curve, nv, nw, n - 1, seed=0x219)
    try:
        r, s = _rs(curve, 24)
        got = backend.groth16_prove(curve.cid, dpk, arrays, z, r, s)
        h_gpu = backend.groth16_last_h(n)
    finally:
        gu.free_pk(backend, dpk)
    exp, h = gu.oracle_prove(curve, arrays, z, hpk, r, s, threads=16, want_h=n)
    assert h[-1].any()
    assert (h_gpu == h).all()
    _same(got, exp)
