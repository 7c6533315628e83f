"""zl_groth16_prove_batch: many proofs over one key and one resident circuit.  Every proof must equal zl_groth16_prove_resident for the same (assignment, r, s)
byte for byte, on the device-batched path (witness map with a batch dimension, A / B / C as three multi-vector MSMs over extended queries; forced here with
ZL_TUNE_G16_BATCH_LOG_N / ZL_TUNE_G16_BATCH_MIN whatever the defaults are) and on the fallback that loops the resident prover."""
import numpy as np
import pytest

import groth16_util as gu
import oracle_lib as ol
import r1cs_gen as rg
from oracle_lib import po
from openzl_amd import ZL_MONT, BackendError, Circuit, Groth16Keys

pytestmark = pytest.mark.gpu
CURVES = [po.BLS12_381, po.BN254]
EINVAL, EHANDLE = -1, -5


def _same(p, q):
    return all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(p, q))


@pytest.fixture
def device_path(monkeypatch):
    monkeypatch.setenv("ZL_TUNE_G16_BATCH_LOG_N", "28")
    monkeypatch.setenv("ZL_TUNE_G16_BATCH_MIN", "1")
    return monkeypatch


def _rs(curve, count, seed):
    rs = ol.random_scalars(curve, 2 * count, seed)
    return np.ascontiguousarray(rs[:count]), np.ascontiguousarray(rs[count:])


@pytest.fixture(scope="module")
def poseidon(backend):
    """per curve: compiled keys of the one-hash Poseidon chain, 130 distinct assignments (another x0 / x1 per proof), distinct (r, s) with r[3] = 0 and s[5] = 0,
    and the resident prover's proof of each -- computed once, shared by the tests below"""
    made = {}

    def get(curve):
        if curve.cid not in made:
            full = Circuit(curve.cid, 1)
            keys = Groth16Keys(backend, full, seed=77)
            zs = []
            for j in range(130):
                c = Circuit(curve.cid, 1, x0=3 + 2 * j, x1=1000 + 7 * j, witness_only=True)
                zs.append(c.arrays()["assignment"])
                c.close()
            Z = np.ascontiguousarray(np.stack(zs))
            r, s = _rs(curve, 130, 501)
            r[3] = 0
            s[5] = 0
            hr = backend.r1cs_upload(curve.cid, full.arrays())
            pk = keys.pk_dict()
            ref = [backend.groth16_prove_resident(curve.cid, pk, hr, Z[j], r[j], s[j]) for j in range(130)]
            made[curve.cid] = (full, keys, Z, r, s, hr, pk, ref)
        return made[curve.cid]

    yield get
    for full, keys, _, _, _, hr, _, _ in made.values():
        backend.r1cs_free(hr)
        keys.close()
        full.close()


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("count", [1, 2, 7, 130])
def test_poseidon_batch_equals_resident_and_verifies(backend, poseidon, device_path, curve, count):
    full, keys, Z, r, s, hr, pk, ref = poseidon(curve)
    assert len({Z[j].tobytes() for j in range(count)}) == count
    got = keys.prove_batch(Z[:count], r[:count], s[:count])
    assert len(got) == count
    for j in range(count):
        assert _same(got[j], ref[j]), j
    ni = full.shape[1]
    assert keys.verify_batch(got, Z[:count, 1:ni])
    with pytest.raises(BackendError) as e:
        backend.groth16_last_h(2)  # no single quotient after a device batch
    assert e.value.code == EINVAL


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_poseidon_paths(backend, poseidon, device_path, curve):
    """Montgomery assignments, a forked lane, several chunks of the prover and of its multi-MSMs, the fallback above the domain bound and below the count bound,
    through the C-ABI binding with a pk dict: always the resident prover's bytes"""
    full, keys, Z, r, s, hr, pk, ref = poseidon(curve)
    count = 7
    fid = 2 if curve.cid == 1 else 4  # the oracle's Fr ids
    Zm = np.zeros_like(Z[:count])
    assert ol.lib().zlo_field_to_mont(fid, ol.p64(np.ascontiguousarray(Z[:count]).reshape(-1)), ol.p64(Zm.reshape(-1)), count * Z.shape[1]) == 0
    check = lambda got: all(_same(got[j], ref[j]) for j in range(count)) and len(got) == count  # noqa: E731
    assert check(backend.groth16_prove_batch(curve.cid, pk, hr, Z[:count], r[:count], s[:count]))
    assert check(backend.groth16_prove_batch(curve.cid, pk, hr, Zm, r[:count], s[:count], flags=ZL_MONT))
    lane = backend.fork()
    try:
        assert check(lane.groth16_prove_batch(curve.cid, pk, hr, Z[:count], r[:count], s[:count]))
        assert check(keys.prove_batch(Z[:count], r[:count], s[:count], lane=lane))
    finally:
        lane.close()
    device_path.setenv("ZL_TUNE_G16_BATCH_CHUNK", "3")      # 3 + 3 + 1 proofs
    assert check(backend.groth16_prove_batch(curve.cid, pk, hr, Z[:count], r[:count], s[:count]))
    device_path.setenv("ZL_TUNE_MSM_MULTI_CHUNK", "2")      # ... each multi-MSM of a chunk in two launch chains
    assert check(backend.groth16_prove_batch(curve.cid, pk, hr, Z[:count], r[:count], s[:count]))
    device_path.delenv("ZL_TUNE_G16_BATCH_CHUNK")
    device_path.delenv("ZL_TUNE_MSM_MULTI_CHUNK")
    n = 1 << max(1, (full.shape[0] + full.shape[1] - 1).bit_length())
    device_path.setenv("ZL_TUNE_G16_BATCH_LOG_N", str(n.bit_length() - 2))  # the domain is one above the bound: the resident prover runs, and leaves its quotient
    assert check(backend.groth16_prove_batch(curve.cid, pk, hr, Z[:count], r[:count], s[:count]))
    assert backend.groth16_last_h(n).shape == (n, 4)
    device_path.setenv("ZL_TUNE_G16_BATCH_LOG_N", "28")
    device_path.setenv("ZL_TUNE_G16_BATCH_MIN", str(count + 1))                # too few proofs for the device path
    assert check(backend.groth16_prove_batch(curve.cid, pk, hr, Z[:count], r[:count], s[:count]))
    assert backend.groth16_last_h(n).shape == (n, 4)


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_nothing_to_prove_and_errors(backend, poseidon, device_path, curve):
    """count == 0, an unknown circuit handle, a query handle of the wrong group, a short key: the resident prover's codes, on the device path and on the fallback"""
    full, keys, Z, r, s, hr, pk, ref = poseidon(curve)
    for log_n in ("28", "0"):
        device_path.setenv("ZL_TUNE_G16_BATCH_LOG_N", log_n)
        assert backend.groth16_prove_batch(curve.cid, pk, hr, Z[:0], r[:0], s[:0]) == []
        with pytest.raises(BackendError) as e:
            backend.groth16_prove_batch(curve.cid, pk, 0x7FFF0001, Z[:2], r[:2], s[:2])
        assert e.value.code == EHANDLE
        with pytest.raises(BackendError) as e:
            backend.groth16_prove_resident(curve.cid, pk, 0x7FFF0001, Z[0], r[0], s[0])
        assert e.value.code == EHANDLE
        bad = dict(pk, b_g2_query=pk["a_query"])
        with pytest.raises(BackendError) as e:
            backend.groth16_prove_batch(curve.cid, bad, hr, Z[:2], r[:2], s[:2])
        assert e.value.code == EHANDLE
        short_h = backend.bases_upload(curve.cid, backend.bases_download(pk["h_query"], 0, 10))
        try:
            short = dict(pk, h_query=short_h)
            with pytest.raises(BackendError) as e:
                backend.groth16_prove_resident(curve.cid, short, hr, Z[0], r[0], s[0])
            assert e.value.code == EINVAL
            with pytest.raises(BackendError) as e:
                backend.groth16_prove_batch(curve.cid, short, hr, Z[:2], r[:2], s[:2])
            assert e.value.code == EINVAL
        finally:
            backend.bases_free(short_h)
    got = backend.groth16_prove_batch(curve.cid, pk, hr, Z[:2], r[:2], s[:2])  # usable after the errors
    assert _same(got[0], ref[0]) and _same(got[1], ref[1])


@pytest.fixture(scope="module")
def random_keys(backend):
    made = {}

    def get(curve):
        if curve.cid not in made:
            hpk = rg.random_key_host(curve, rg.KEY_NV, rg.KEY_NW, rg.KEY_NH, seed=0x7A7A + curve.cid)
            made[curve.cid] = (gu.upload_pk(backend, curve, hpk), hpk)
        return made[curve.cid]

    yield get
    for dpk, _ in made.values():
        gu.free_pk(backend, dpk)


@pytest.mark.parametrize("name", ["smallest", "full16", "full17", "many_publics", "no_witness", "sparse_a", "long_c", "mixed", "unsat_mixed"])
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_generic_shapes_batch_of_five(backend, random_keys, device_path, curve, name):
    """assignment 0 = the circuit's own (proof 0 also equals the oracle's), assignments 1..4 random vectors with z[0] = 1: a proof is a function of (z, r, s)
    whether or not z satisfies the circuit.  One key of random points serves every shape (the extended queries are rebuilt when the shape changes)."""
    cs, arrays = rg.shape_case(curve, name)
    dpk, hpk = random_keys(curve)
    nv = cs.n_instance + cs.n_witness
    count = 5
    Z = np.zeros((count, nv, 4), dtype=np.uint64)
    Z[0] = ol.ints_to_limbs(cs.assignment(), 4)
    Z[1:] = ol.random_scalars(curve, (count - 1) * nv, 900 + nv).reshape(count - 1, nv, 4)
    Z[1:, 0] = ol.ints_to_limbs([1], 4)[0]
    r, s = _rs(curve, count, 901 + nv)
    hr = backend.r1cs_upload(curve.cid, arrays)
    try:
        got = backend.groth16_prove_batch(curve.cid, dpk, hr, Z, r, s)
        ref = [backend.groth16_prove_resident(curve.cid, dpk, hr, Z[j], r[j], s[j]) for j in range(count)]
    finally:
        backend.r1cs_free(hr)
    for j in range(count):
        assert _same(got[j], ref[j]), j
    exp, _ = gu.oracle_prove(curve, arrays, Z[0], hpk, r[0], s[0], threads=8)
    assert _same(got[0], exp)
