"""Batched Groth16 verification on the device (zl_groth16_verify_batch): valid batches of device-made Poseidon proofs and of oracle-made proofs of generic
R1CS shapes are accepted; verdicts equal per-proof zl_groth16_verify and the host implementation of the same random linear combination
(zl_test_verify_batch_host); tampered batches are rejected with exactly the tampered proofs marked; NULL seed, empty batches, a wrong n_public and a key
round-tripped through its wire format behave."""
import numpy as np
import pytest

import batch_verify_util as bv
from oracle_lib import po
from openzl_amd import Circuit, Groth16Keys
from openzl_amd.backend import BackendError, hook_verify_batch_host

CURVES = [po.BLS12_381, po.BN254]


def _vk_points(keys, curve, circ):
    """verifying key of device keys as canonical points, for the host hook: recomputed from the trapdoor exponents"""
    import groth16_util as gu
    import oracle_lib as ol

    al, be, ga, de, tau = keys.trapdoor()
    cs = po.poseidon_chain_circuit(curve.fr, 1)
    ex = po.groth16_setup_exponents(curve, cs, po.Groth16Trapdoor(alpha=al, beta=be, gamma=ga, delta=de, tau=tau))
    return {"alpha_g1": ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs([al], 4))[0], "beta_g2": gu.g2_mul_gen(curve, [be])[0],
            "gamma_g2": gu.g2_mul_gen(curve, [ga])[0], "delta_g2": gu.g2_mul_gen(curve, [de])[0],
            "gamma_abc": ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs(ex["gamma_abc"], 4))}


@pytest.fixture(scope="module", params=CURVES, ids=lambda c: c.name)
def poseidon(request, backend):
    curve = request.param
    circ = Circuit(curve.cid, 1)
    keys = Groth16Keys(backend, circ, seed=0xB47C4)
    proofs = keys.prove_many(list(range(1000, 2000)))
    pub = circ.arrays()["assignment"][1:2]
    yield curve, circ, keys, proofs, pub
    keys.close()


@pytest.mark.gpu
def test_poseidon_batches_accepted_and_match_per_proof_and_host(poseidon):
    curve, circ, keys, proofs, pub = poseidon
    vk = _vk_points(keys, curve, circ)
    for count in (1, 2, 7, 64, 1000):
        pubs = np.tile(pub[None], (count, 1, 1))
        ok, each = keys.verify_batch(proofs[:count], pubs, seed=7, each=True)
        assert ok and each.all(), count
        if count <= 64:
            assert all(keys.verify(p, pub) for p in proofs[:count])
            hok, heach = hook_verify_batch_host(curve.cid, vk, proofs[:count], pubs, 1, seed=7)
            assert hok and (heach == each).all()
    assert keys.verify_batch(proofs[:5], np.tile(pub[None], (5, 1, 1))) is True  # seed from the OS
    assert keys.verify_batch([], np.zeros((0, 1, 4), dtype=np.uint64)) is True


@pytest.mark.gpu
@pytest.mark.parametrize("how", bv.TAMPER_CASES + ["offcurve_b"])
def test_tampered_batches_rejected_with_exact_verdicts(poseidon, how):
    curve, circ, keys, proofs, pub = poseidon
    vk = _vk_points(keys, curve, circ)
    pubs = np.tile(pub[None], (8, 1, 1))
    bad, bpubs, idx = bv.tampered(curve, proofs[:8], pubs, how)
    ok, each = keys.verify_batch(bad, bpubs, seed=3, each=True)
    assert not ok
    assert [bool(e) for e in each] == [i not in idx for i in range(8)]
    assert [bool(e) for e in each] == [keys.verify(bad[i], bpubs[i]) for i in range(8)]
    hok, heach = hook_verify_batch_host(curve.cid, vk, bad, bpubs, 1, seed=3)
    assert hok is False and (heach == each).all()


@pytest.mark.gpu
def test_duplicates_wrong_n_public_and_key_round_trip(poseidon, backend):
    curve, circ, keys, proofs, pub = poseidon
    dup = [proofs[0], proofs[0], proofs[1]]
    assert keys.verify_batch(dup, np.tile(pub[None], (3, 1, 1)), seed=1) is True
    with pytest.raises(BackendError) as e:
        keys.verify_batch(proofs[:2], np.zeros((2, 2, 4), dtype=np.uint64), seed=1)
    assert e.value.code == -1
    k2 = Groth16Keys.from_bytes(backend, circ, keys.to_bytes())
    try:
        ok, each = k2.verify_batch(proofs[:64], np.tile(pub[None], (64, 1, 1)), seed=9, each=True)
        assert ok and each.all()
    finally:
        k2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("kind", ["smallest", "many_publics"])
def test_generic_shapes_oracle_proofs(backend, curve, kind):
    case = bv.Case(curve, kind)
    proofs = case.proofs(64, seed=4)
    k = bv.oracle_keys(backend, case)
    try:
        for count in (1, 7, 64):
            pubs = case.pubs(count)
            ok, each = bv.verify_raw(backend, k, proofs[:count], pubs, case.n_public, seed=11)
            assert ok and each.all(), count
            hok, heach = hook_verify_batch_host(curve.cid, case.vk, proofs[:count], pubs, case.n_public, seed=11)
            assert hok and (heach == each).all()
        bad, bpubs, idx = bv.tampered(curve, proofs[:7], case.pubs(7), "public" if case.n_public else "swap_c")
        ok, each = bv.verify_raw(backend, k, bad, bpubs, case.n_public, seed=11)
        assert not ok and [bool(e) for e in each] == [i not in idx for i in range(7)]
    finally:
        backend.L.zl_groth16_keys_free(k)
