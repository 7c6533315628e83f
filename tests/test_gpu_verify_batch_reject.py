"""Rejected batches of zl_groth16_verify_batch with per-proof verdicts from DEVICE final exponentiations (ZL_TUNE_FEXP_DEV_MIN = 1, three values per launch):
235-constraint Poseidon proofs in batches of 5, 64 and 70 with the first, the last or several proofs tampered (A taken from another proof, a wrong C, a wrong
public input, A at infinity).  The verdicts equal the host implementation of the same batch (zl_test_verify_batch_host), the host-thread path of the same
entry point (ZL_TUNE_FEXP_DEV_MIN very large) and the set of tampered indices; once through the bytes-in verifier.  B or C at infinity (zero words and
the flag) on each of those paths and over several launch sets (ZL_TUNE_PAIR_SET), and a rejected batch under a combination drawn from the OS."""
import numpy as np
import pytest

import batch_verify_util as bv
import groth16_util as gu
import oracle_lib as ol
from oracle_lib import po
from openzl_amd import Circuit, Groth16Keys
from openzl_amd.backend import hook_verify_batch_host, proof_to_bytes

pytestmark = pytest.mark.gpu

CURVES = [po.BLS12_381, po.BN254]
N = 70
HOST_ONLY = 1 << 30  # a chunk never holds that many proofs: the host threads


@pytest.fixture(scope="module", params=CURVES, ids=lambda c: c.name)
def poseidon(request, backend):
    curve = request.param
    circ = Circuit(curve.cid, 1)
    keys = Groth16Keys(backend, circ, seed=0xFE7C4)
    proofs = keys.prove_many(list(range(3000, 3000 + N)))
    pub = circ.arrays()["assignment"][1:2]
    al, be, ga, de, tau = keys.trapdoor()
    ex = po.groth16_setup_exponents(curve, po.poseidon_chain_circuit(curve.fr, 1), po.Groth16Trapdoor(alpha=al, beta=be, gamma=ga, delta=de, tau=tau))
    vk = {"alpha_g1": ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs([al], 4))[0], "beta_g2": gu.g2_mul_gen(curve, [be])[0],
          "gamma_g2": gu.g2_mul_gen(curve, [ga])[0], "delta_g2": gu.g2_mul_gen(curve, [de])[0],
          "gamma_abc": ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs(ex["gamma_abc"], 4))}
    yield curve, keys, proofs, pub, vk
    keys.close()


def _tamper(proofs, pubs, plan):
    """plan: index -> kind.  Every kind changes the proof at that index alone (the donor of an A or a C is left as it is)."""
    n = len(proofs)
    proofs = [tuple(np.array(x, copy=True) if isinstance(x, np.ndarray) else x for x in p) for p in proofs]
    pubs = np.array(pubs, copy=True)
    for i, kind in plan.items():
        p, donor = list(proofs[i]), proofs[(i + 1) % n]
        if kind == "other_a":
            p[0] = donor[0].copy()
        elif kind == "wrong_c":
            p[4] = donor[4].copy()
        elif kind == "public":
            pubs[i, 0, 0] ^= np.uint64(1)
        elif kind == "a_inf":
            p[0], p[1] = np.zeros_like(p[0]), 1
        else:
            raise ValueError(kind)
        proofs[i] = tuple(p)
    return proofs, pubs


def _with_env(dev_min, chunk, fn):
    return _with_vars({"ZL_TUNE_FEXP_DEV_MIN": dev_min, "ZL_TUNE_FEXP_CHUNK": chunk}, fn)


_with_vars = bv.with_vars


SCENARIOS = [
    (5, {0: "other_a"}),
    (5, {4: "a_inf"}),
    (64, {63: "wrong_c"}),
    (64, {0: "public"}),
    (70, {0: "a_inf", 13: "public", 37: "other_a", 64: "wrong_c", 69: "other_a"}),
]


@pytest.mark.parametrize("count,plan", SCENARIOS, ids=lambda v: str(v) if isinstance(v, int) else "+".join(f"{i}{k}" for i, k in v.items()))
def test_device_verdicts_equal_the_host(poseidon, count, plan):
    curve, keys, proofs, pub, vk = poseidon
    bad, bpubs = _tamper(proofs[:count], np.tile(pub[None], (count, 1, 1)), plan)
    expected = [i not in plan for i in range(count)]
    hok, heach = hook_verify_batch_host(curve.cid, vk, bad, bpubs, 1, seed=13)
    assert hok is False and [bool(e) for e in heach] == expected
    ok, each = _with_env(1, 3, lambda: keys.verify_batch(bad, bpubs, seed=13, each=True))
    assert ok is False
    assert each.tobytes() == heach.tobytes()
    ok2, each2 = _with_env(HOST_ONLY, 3, lambda: keys.verify_batch(bad, bpubs, seed=13, each=True))
    assert ok2 is False and each2.tobytes() == each.tobytes()


@pytest.mark.parametrize("how", bv.INF_CASES)
def test_b_or_c_at_infinity_rejects_that_proof_on_every_path(poseidon, how):
    """B or C of one proof of three as a decoder hands over infinity (zero words, flag set): device final exponentiations, host threads, and two launch
    sets of the combined product with one proof per reject-path set; the verdicts are the host implementation's and zl_groth16_verify's"""
    curve, keys, proofs, pub, vk = poseidon
    bad, bpubs, idx = bv.tampered(curve, proofs[:3], np.tile(pub[None], (3, 1, 1)), how)
    expected = [i not in idx for i in range(3)]
    hok, heach = hook_verify_batch_host(curve.cid, vk, bad, bpubs, 1, seed=17)
    assert hok is False and [bool(e) for e in heach] == expected
    assert [keys.verify(bad[i], bpubs[i]) for i in range(3)] == expected
    for env in ({"ZL_TUNE_FEXP_DEV_MIN": 1}, {"ZL_TUNE_FEXP_DEV_MIN": HOST_ONLY}, {"ZL_TUNE_PAIR_SET": 4}):
        ok, each = _with_vars(env, lambda: keys.verify_batch(bad, bpubs, seed=17, each=True))
        assert ok is False, env
        assert each.tobytes() == heach.tobytes(), env


def test_combination_drawn_from_the_os_rejects_with_exact_verdicts(poseidon):
    """no seed: rho comes from getrandom.  No tolerance: a 128-bit combination accepts a bad batch with probability 2^-128, and the per-proof verdicts
    do not depend on rho at all"""
    curve, keys, proofs, pub, vk = poseidon
    bad, bpubs = _tamper(proofs[:5], np.tile(pub[None], (5, 1, 1)), {2: "public"})
    ok, each = keys.verify_batch(bad, bpubs, each=True)
    assert ok is False
    assert [bool(e) for e in each] == [i != 2 for i in range(5)]


def test_bytes_in_verifier_takes_the_device_path(poseidon):
    curve, keys, proofs, pub, vk = poseidon
    plan = {0: "wrong_c", 6: "a_inf", 69: "public"}
    bad, bpubs = _tamper(proofs, np.tile(pub[None], (N, 1, 1)), plan)
    data = b"".join(proof_to_bytes(curve.cid, p) for p in bad)
    hok, heach = hook_verify_batch_host(curve.cid, vk, bad, bpubs, 1, seed=21)
    ok, each, st = _with_env(1, 3, lambda: keys.verify_batch_bytes(data, N, bpubs, seed=21, each=True))
    assert ok is False and hok is False and not st.any()
    assert each.tobytes() == heach.tobytes() and [bool(e) for e in each] == [i not in plan for i in range(N)]
    ok2, each2, _ = _with_env(HOST_ONLY, 3, lambda: keys.verify_batch_bytes(data, N, bpubs, seed=21, each=True))
    assert ok2 is False and each2.tobytes() == each.tobytes()
