"""zl_groth16_prove_batch_dev (assignments in device memory) and zl_groth16_prove_poseidon_chains (chain inputs in, proofs out: the trace kernel writes the
assignments straight into the batch's block).  Every proof must equal zl_groth16_prove_resident for the same (assignment, r, s) byte for byte, on the device
path (forced with ZL_TUNE_G16_BATCH_LOG_N / _MIN) and on both fallbacks to the loop over the resident prover; the public inputs must be the chain digests."""
import numpy as np
import pytest

import oracle_lib as ol
import poseidon_util as pu
from openzl_amd import ZL_MONT, BackendError, Circuit, Groth16Keys

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
EINVAL, EHANDLE = -1, -5


def _same(p, q):
    return all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(p, q))


def dev(a: np.ndarray):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


@pytest.fixture
def device_path(monkeypatch):
    monkeypatch.setenv("ZL_TUNE_G16_BATCH_LOG_N", "28")
    monkeypatch.setenv("ZL_TUNE_G16_BATCH_MIN", "1")
    monkeypatch.setenv("ZL_TUNE_POSEIDON_DEV_MIN", "0")
    return monkeypatch


def _make(backend, curve, k, count, seed):
    """keys of the k-link chain, `count` distinct input pairs with the witness-only compilers' assignments, distinct (r, s) with one zero each, and the
    resident prover's proof of each"""
    full = Circuit(curve.cid, k)
    keys = Groth16Keys(backend, full, seed=seed)
    x0 = [3 + 2 * j for j in range(count)]
    x1 = [1000 + 7 * j for j in range(count)]
    x0[1], x1[2] = curve.fr.p - 1, 0
    zs = []
    for a, b in zip(x0, x1):
        c = Circuit(curve.cid, k, x0=a, x1=b, witness_only=True)
        zs.append(c.arrays()["assignment"])
        c.close()
    Z = np.ascontiguousarray(np.stack(zs))
    rs = ol.random_scalars(curve, 2 * count, seed + 1)
    r, s = np.ascontiguousarray(rs[:count]), np.ascontiguousarray(rs[count:])
    r[min(3, count - 1)] = 0
    s[min(4, count - 1)] = 0
    hr = backend.r1cs_upload(curve.cid, full.arrays())
    pk = keys.pk_dict()
    ref = [backend.groth16_prove_resident(curve.cid, pk, hr, Z[j], r[j], s[j]) for j in range(count)]
    return dict(full=full, keys=keys, x0=pu.limbs(x0), x1=pu.limbs(x1), Z=Z, r=r, s=s, hr=hr, pk=pk, ref=ref, k=k)


def _drop(backend, made):
    for m in made.values():
        backend.r1cs_free(m["hr"])
        m["keys"].close()
        m["full"].close()


@pytest.fixture(scope="module")
def chain1(backend):
    """per curve: the one-link chain with 130 proofs' worth of references, computed once and shared"""
    made = {}

    def get(curve):
        if curve.cid not in made:
            made[curve.cid] = _make(backend, curve, 1, 130, 771)
        return made[curve.cid]

    yield get
    _drop(backend, made)


def _check(m, got, count):
    return len(got) == count and all(_same(got[j], m["ref"][j]) for j in range(count))


def _fallbacks(m, device_path):
    """the two settings that send a batch of 7 to the loop over the resident prover"""
    n = 1 << max(1, (m["full"].shape[0] + m["full"].shape[1] - 1).bit_length())
    yield {"ZL_TUNE_G16_BATCH_LOG_N": str(n.bit_length() - 2), "ZL_TUNE_G16_BATCH_MIN": "1"}  # the domain bound below the circuit
    yield {"ZL_TUNE_G16_BATCH_LOG_N": "28", "ZL_TUNE_G16_BATCH_MIN": "8"}                       # the minimum count above the batch


# ---- assignments in device memory ----------------------------------------------------------------------------------------------------------------------
@CURVES
@pytest.mark.parametrize("count", [1, 7, 130])
def test_prove_batch_dev_equals_resident(backend, chain1, device_path, curve, count):
    m = chain1(curve)
    d_z = dev(m["Z"][:count])
    got = m["keys"].prove_batch_dev(d_z.data_ptr(), count, m["r"][:count], m["s"][:count])
    assert _check(m, got, count)
    with pytest.raises(BackendError) as e:
        backend.groth16_last_h(2)  # the device path ran: no single quotient
    assert e.value.code == EINVAL


@CURVES
def test_prove_batch_dev_paths(backend, chain1, device_path, curve):
    m = chain1(curve)
    count = 7
    Z, r, s, pk, hr = m["Z"][:count], m["r"][:count], m["s"][:count], m["pk"], m["hr"]
    fid = 2 if curve.cid == 1 else 4  # the oracle's Fr ids
    Zm = np.zeros_like(Z)
    assert ol.lib().zlo_field_to_mont(fid, ol.p64(np.ascontiguousarray(Z).reshape(-1)), ol.p64(Zm.reshape(-1)), count * Z.shape[1]) == 0
    d_z, d_zm = dev(Z), dev(Zm)
    assert _check(m, backend.groth16_prove_batch_dev(curve.cid, pk, hr, d_z.data_ptr(), count, r, s), count)
    assert _check(m, backend.groth16_prove_batch_dev(curve.cid, pk, hr, d_zm.data_ptr(), count, r, s, flags=ZL_MONT), count)
    device_path.setenv("ZL_TUNE_G16_BATCH_CHUNK", "3")  # 3 + 3 + 1 proofs
    assert _check(m, backend.groth16_prove_batch_dev(curve.cid, pk, hr, d_z.data_ptr(), count, r, s), count)
    device_path.delenv("ZL_TUNE_G16_BATCH_CHUNK")
    n = 1 << max(1, (m["full"].shape[0] + m["full"].shape[1] - 1).bit_length())
    for env in _fallbacks(m, device_path):
        for key, v in env.items():
            device_path.setenv(key, v)
        assert _check(m, backend.groth16_prove_batch_dev(curve.cid, pk, hr, d_z.data_ptr(), count, r, s), count)
        assert backend.groth16_last_h(n).shape == (n, 4)  # the resident prover ran and left its quotient
        assert _check(m, backend.groth16_prove_batch_dev(curve.cid, pk, hr, d_zm.data_ptr(), count, r, s, flags=ZL_MONT), count)
    assert backend.groth16_prove_batch_dev(curve.cid, pk, hr, 0, 0, r[:0], s[:0]) == []
    with pytest.raises(BackendError) as e:
        backend.groth16_prove_batch_dev(curve.cid, pk, 0x7FFF0001, d_z.data_ptr(), count, r, s)
    assert e.value.code == EHANDLE


# ---- chain inputs in, proofs out -----------------------------------------------------------------------------------------------------------------------
@CURVES
@pytest.mark.parametrize("count", [1, 7, 130])
def test_prove_chains_equals_resident_and_verifies(backend, chain1, device_path, curve, count):
    m = chain1(curve)
    got, pub = m["keys"].prove_chains(m["x0"][:count], m["x1"][:count], m["r"][:count], m["s"][:count])
    assert _check(m, got, count)
    assert np.array_equal(pub, backend.poseidon_chain(curve.cid, m["x0"][:count], m["x1"][:count], 1))
    assert np.array_equal(pub, m["Z"][:count, 1])
    assert m["keys"].verify_batch(got, pub.reshape(count, 1, 4))


@CURVES
def test_prove_chains_two_links(backend, device_path, curve):
    made = {0: _make(backend, curve, 2, 5, 881)}
    try:
        m = made[0]
        assert m["keys"].chain_links() == 2
        got, pub = m["keys"].prove_chains(m["x0"], m["x1"], m["r"], m["s"])
        assert _check(m, got, 5)
        assert np.array_equal(pub, backend.poseidon_chain(curve.cid, m["x0"], m["x1"], 2))
        assert m["keys"].verify_batch(got, pub.reshape(5, 1, 4))
        device_path.setenv("ZL_TUNE_G16_BATCH_CHUNK", "2")
        device_path.setenv("ZL_TUNE_POSEIDON_CHUNK", "1")
        got2, pub2 = m["keys"].prove_chains(m["x0"], m["x1"], m["r"], m["s"])
        assert _check(m, got2, 5) and np.array_equal(pub2, pub)
    finally:
        _drop(backend, made)


@CURVES
def test_prove_chains_paths(backend, chain1, device_path, curve):
    """several chunks of the prover, each of several launches of the trace kernel; a forked lane; both fallbacks"""
    m = chain1(curve)
    count = 7
    x0, x1, r, s = m["x0"][:count], m["x1"][:count], m["r"][:count], m["s"][:count]
    exp_pub = m["Z"][:count, 1]
    device_path.setenv("ZL_TUNE_G16_BATCH_CHUNK", "3")   # 3 + 3 + 1 proofs ...
    device_path.setenv("ZL_TUNE_POSEIDON_CHUNK", "2")    # ... whose chains run as 2 + 1, 2 + 1 and 1
    got, pub = m["keys"].prove_chains(x0, x1, r, s)
    assert _check(m, got, count) and np.array_equal(pub, exp_pub)
    assert m["keys"].verify_batch(got, pub.reshape(count, 1, 4))
    device_path.delenv("ZL_TUNE_G16_BATCH_CHUNK")
    device_path.delenv("ZL_TUNE_POSEIDON_CHUNK")
    lane = backend.fork()
    try:
        got, pub = m["keys"].prove_chains(x0, x1, r, s, lane=lane)
        assert _check(m, got, count) and np.array_equal(pub, exp_pub)
    finally:
        lane.close()
        backend._forks.remove(lane)
    n = 1 << max(1, (m["full"].shape[0] + m["full"].shape[1] - 1).bit_length())
    for env in _fallbacks(m, device_path):
        for key, v in env.items():
            device_path.setenv(key, v)
        for dev_min in ("0", str(1 << 30)):  # the assignments of the fallback from the device, and from the host mirror
            device_path.setenv("ZL_TUNE_POSEIDON_DEV_MIN", dev_min)
            got, pub = m["keys"].prove_chains(x0, x1, r, s)
            assert _check(m, got, count) and np.array_equal(pub, exp_pub)
            assert backend.groth16_last_h(n).shape == (n, 4)


@CURVES
def test_prove_chains_errors(backend, chain1, device_path, curve):
    m = chain1(curve)
    x0, x1, r, s, pk, hr = m["x0"][:4], m["x1"][:4], m["r"][:4], m["s"][:4], m["pk"], m["hr"]
    for log_n in ("28", "0"):  # on the device path and on the fallback
        device_path.setenv("ZL_TUNE_G16_BATCH_LOG_N", log_n)
        with pytest.raises(BackendError) as e:
            backend.groth16_prove_poseidon_chains(curve.cid, pk, hr, 2, x0, x1, r, s)  # a 2-link chain against the 1-link circuit
        assert e.value.code == EINVAL
        with pytest.raises(BackendError) as e:
            backend.groth16_prove_poseidon_chains(curve.cid, pk, hr, 0, x0, x1, r, s)
        assert e.value.code == EINVAL
        with pytest.raises(BackendError) as e:
            backend.groth16_prove_poseidon_chains(curve.cid, pk, 0x7FFF0001, 1, x0, x1, r, s)
        assert e.value.code == EHANDLE
        bad = x1.copy()
        bad[2] = pu.limbs([curve.fr.p])[0]
        with pytest.raises(BackendError) as e:
            m["keys"].prove_chains(x0, bad, r, s)
        assert e.value.code == EINVAL
        got, pub = m["keys"].prove_chains(x0[:0], x1[:0], r[:0], s[:0])
        assert got == [] and pub.shape == (0, 4)
        got, pub = backend.groth16_prove_poseidon_chains(curve.cid, pk, hr, 1, x0, x1, r, s)  # usable after the errors
        assert _check(m, got, 4) and np.array_equal(pub, m["Z"][:4, 1])


def test_keys_of_another_circuit_are_refused(chain1, monkeypatch):
    """prove_chains derives k from the shape of the keys' circuit and refuses a shape that is no chain before it calls the library.  This backend builds no
    circuit but the chain, so the refusal is reached with a stand-in for the keys' public `circuit` attribute; the library's own shape check is the k = 2 case
    of test_prove_chains_errors."""
    m = chain1(pu.CURVES[0])
    keys = m["keys"]
    assert keys.chain_links() == 1

    class NotAChain:
        curve = keys.circuit.curve
        shape = (235, 2, 235)  # one witness short of the one-link chain

    monkeypatch.setattr(keys, "circuit", NotAChain())
    assert keys.chain_links() == 0
    with pytest.raises(ValueError):
        keys.prove_chains(m["x0"][:1], m["x1"][:1], m["r"][:1], m["s"][:1])
