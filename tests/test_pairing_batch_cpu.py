"""Batched Groth16 verification, host half (no GPU): zl_test_verify_batch_host runs zl_groth16_verify_batch's random linear combination -- rho derivation,
aggregated public-input point, shared beta / gamma / delta pairs, infinity rules, per-proof fallback -- over the host lock-step multi-pairing.  Proofs come from
the oracle under a fixed trapdoor (Poseidon chain and generic R1CS shapes); per-proof verdicts are checked against the definition-level Python pairing."""
import pytest

import batch_verify_util as bv
from oracle_lib import po
from openzl_amd.backend import BackendError, hook_verify_batch_host

CURVES = [po.BLS12_381, po.BN254]
_CASES = {}


def _case(curve, kind):
    key = (curve.cid, kind)
    if key not in _CASES:
        c = bv.Case(curve, kind)
        _CASES[key] = (c, c.proofs(7))
    return _CASES[key]


def _run(case, proofs, pubs, seed=5):
    return hook_verify_batch_host(case.curve.cid, case.vk, proofs, pubs, case.n_public, seed=seed)


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("kind", ["poseidon", "smallest", "many_publics"])
def test_host_batch_accepts_valid_batches(curve, kind):
    case, proofs = _case(curve, kind)
    for count in (1, 2, 7):
        ok, each = _run(case, proofs[:count], case.pubs(count))
        assert ok and each.all(), (kind, count)
    ok, each = _run(case, [], case.pubs(0))
    assert ok and len(each) == 0


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("how", bv.TAMPER_CASES + bv.INF_CASES)
def test_host_batch_rejects_tampering_with_per_proof_verdicts(curve, how):
    case, proofs = _case(curve, "poseidon")
    bad, pubs, idx = bv.tampered(curve, proofs[:3], case.pubs(3), how)
    ok, each = _run(case, bad, pubs)
    assert not ok
    assert [bool(e) for e in each] == [i not in idx for i in range(3)]
    # each verdict is the definition-level Groth16 verification of that proof
    assert [bool(e) for e in each] == [case.py_verify(bad[i], pubs[i]) for i in range(3)]
    # the verdicts do not depend on the combination's seed
    ok2, each2 = _run(case, bad, pubs, seed=0xDEADBEEF)
    assert ok2 == ok and (each2 == each).all()


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_host_batch_rejects_under_a_combination_drawn_from_the_os(curve):
    """no seed: rho comes from getrandom.  No tolerance: a 128-bit combination accepts a bad batch with probability 2^-128, and the per-proof verdicts
    do not depend on rho at all"""
    case, proofs = _case(curve, "poseidon")
    bad, pubs, idx = bv.tampered(curve, proofs[:5], case.pubs(5), "public")
    ok, each = _run(case, bad, pubs, seed=None)
    assert not ok
    assert [bool(e) for e in each] == [i not in idx for i in range(5)]


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_host_batch_seeds_and_arguments(curve):
    case, proofs = _case(curve, "many_publics")
    for seed in (1, 2, None):
        ok, each = _run(case, proofs[:3], case.pubs(3), seed=seed)
        assert ok and each.all()
    # the hook takes gamma_abc as n_public + 1 points; an unknown curve is refused (the key-based zl_groth16_verify_batch checks n_public against the key:
    # tests/test_gpu_groth16_verify_batch.py)
    with pytest.raises(BackendError) as e:
        hook_verify_batch_host(3, case.vk, proofs[:2], case.pubs(2), case.n_public, seed=1)
    assert e.value.code == -1  # ZL_EINVAL
