"""The device final exponentiation (k_pd_fexp of csrc/zl_pairing_dev.hip, through zl_test_final_exp_dev) against the host's Engine::final_exp
(zl_test_final_exp), bit for bit: random general Fq12 elements at counts that cross the four-group block and the 64-lane wave; one batch that mixes one, an
element of Fq, zero and raw device Miller values (one with P at infinity) among random values; a chunked run equal to the single launch."""
import os
import random

import numpy as np
import pytest

import groth16_util as gu
import oracle_lib as ol
from oracle_lib import po
from openzl_amd import pairing
from openzl_amd.backend import BackendError, hook_final_exp, hook_final_exp_dev, hook_miller_dev

pytestmark = pytest.mark.gpu

CURVES = [po.BLS12_381, po.BN254]
ENOTCURVE = -6
_cache = {}


def _random_values(curve):
    """65 random general elements of Fq12 and their host final exponentiations, computed once per curve"""
    if curve.cid not in _cache:
        rng = random.Random(0xFE0 + curve.cid)
        q, nq = curve.fq.p, ol.nlq(curve)
        vals = np.stack([ol.ints_to_limbs([rng.randrange(q) for _ in range(12)], nq) for _ in range(65)])
        exp = np.stack([hook_final_exp(curve.cid, v) for v in vals])
        vals.setflags(write=False)
        exp.setflags(write=False)
        _cache[curve.cid] = (vals, exp)
    return _cache[curve.cid]


def _elem(curve, coeffs):
    return ol.ints_to_limbs(list(coeffs) + [0] * (12 - len(coeffs)), ol.nlq(curve))


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("count", [1, 3, 4, 5, 64, 65])
def test_random_values_equal_the_host(backend, curve, count):
    vals, exp = _random_values(curve)
    got, singular = hook_final_exp_dev(backend, curve.cid, vals[:count])
    assert got.shape == (count, 12, ol.nlq(curve)) and not singular.any()
    bad = [i for i in range(count) if (got[i] != exp[i]).any()]
    assert not bad, bad


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_mixed_batch_special_values_and_miller_values(backend, curve):
    vals, exp = _random_values(curve)
    P = ol.oracle_g1_mul_gen(curve, ol.random_scalars(curve, 3, 71))
    Q = gu.g2_mul_gen(curve, ol.limbs_to_ints(ol.random_scalars(curve, 3, 72)))
    P[1] = 0  # infinity: a Miller value of one
    raw = hook_miller_dev(backend, curve.cid, P, Q)
    one, zero = _elem(curve, [1]), _elem(curve, [])
    fq = _elem(curve, [0x1234_5678_9ABC_DEF0_1357])
    # position -> value; the random values in between must come out as they do alone
    batch = [vals[0], one, vals[1], fq, zero, vals[2], raw[0], raw[1], vals[3], raw[2], vals[4]]
    got, singular = hook_final_exp_dev(backend, curve.cid, np.stack(batch))
    assert list(singular) == [1 if i == 4 else 0 for i in range(len(batch))]
    for pos, k in ((0, 0), (2, 1), (5, 2), (8, 3), (10, 4)):
        assert (got[pos] == exp[k]).all(), pos
    assert (got[1] == one).all() and (hook_final_exp(curve.cid, one) == one).all()
    assert (got[3] == one).all() and (hook_final_exp(curve.cid, fq) == one).all()
    # zero: the host reports it (ZL_ENOTCURVE) and leaves zero
    assert (got[4] == zero).all()
    with pytest.raises(BackendError) as e:
        hook_final_exp(curve.cid, zero)
    assert e.value.code == ENOTCURVE
    for pos, i in ((6, 0), (7, 1), (9, 2)):
        assert (got[pos] == pairing(curve.cid, P[i], Q[i])).all(), pos
        assert (got[pos] == hook_final_exp(curve.cid, raw[i])).all(), pos
    assert (got[7] == one).all()


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_chunked_launches_give_the_bytes_of_one_launch(backend, curve):
    vals, exp = _random_values(curve)
    batch = np.array(vals[:10])
    batch[6] = 0  # the singular flags are chunked with the values
    whole, s_whole = hook_final_exp_dev(backend, curve.cid, batch)
    old = os.environ.get("ZL_TUNE_FEXP_CHUNK")
    os.environ["ZL_TUNE_FEXP_CHUNK"] = "3"  # 3 + 3 + 3 + 1
    try:
        parts, s_parts = hook_final_exp_dev(backend, curve.cid, batch)
    finally:
        if old is None:
            del os.environ["ZL_TUNE_FEXP_CHUNK"]
        else:
            os.environ["ZL_TUNE_FEXP_CHUNK"] = old
    assert whole.tobytes() == parts.tobytes() and s_whole.tobytes() == s_parts.tobytes()
    assert list(s_whole) == [1 if i == 6 else 0 for i in range(10)]
    assert all((whole[i] == exp[i]).all() for i in range(10) if i != 6)
