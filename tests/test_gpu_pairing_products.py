"""Many independent pairing products in one call (zl_pairing_products: device Miller loops in groups, device final exponentiations): every row equals
zl_pairing_product over that product's pairs; a product that is one, pairs with a point at infinity, the empty batch, empty products, the pairs_each limit, and
a run chunked over several launch sets equal to the unchunked one."""
import os

import numpy as np
import pytest

import groth16_util as gu
import oracle_lib as ol
from oracle_lib import po
from openzl_amd.backend import BackendError

pytestmark = pytest.mark.gpu

CURVES = [po.BLS12_381, po.BN254]
MAX_PAIRS = 1 << 16
EINVAL = -1
ENOTCURVE = -6
_cache = {}


def _pairs(curve):
    """130 pairs (a_i G1, b_i G2), generated once per curve"""
    if curve.cid not in _cache:
        P = ol.oracle_g1_mul_gen(curve, ol.random_scalars(curve, 130, 81))
        Q = gu.g2_mul_gen(curve, ol.limbs_to_ints(ol.random_scalars(curve, 130, 82)))
        P.setflags(write=False)
        Q.setflags(write=False)
        _cache[curve.cid] = (P, Q)
    return _cache[curve.cid]


def _one(curve):
    return ol.ints_to_limbs([1] + [0] * 11, ol.nlq(curve))


def _with_chunk(value, fn):
    old = os.environ.get("ZL_TUNE_FEXP_CHUNK")
    os.environ["ZL_TUNE_FEXP_CHUNK"] = str(value)
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["ZL_TUNE_FEXP_CHUNK"]
        else:
            os.environ["ZL_TUNE_FEXP_CHUNK"] = old


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("count,each", [(1, 1), (5, 1), (3, 4), (65, 2), (2, 33)])
def test_rows_equal_single_products(backend, curve, count, each):
    P, Q = _pairs(curve)
    P, Q = P[:count * each], Q[:count * each]
    got, status = backend.pairing_products(curve.cid, P, Q, each)
    assert got.shape == (count, 12, ol.nlq(curve)) and status.shape == (count,) and not status.any()
    for j in range(count):
        exp = backend.pairing_product(curve.cid, P[j * each:(j + 1) * each], Q[j * each:(j + 1) * each])
        assert (got[j] == exp).all(), j


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_a_product_that_is_one_and_pairs_at_infinity(backend, curve):
    r = curve.fr.p
    a = 0x5EED5EED5EED
    P, Q = (np.array(x[:10]) for x in _pairs(curve))
    # product 2 = e(aP, Q) e(P, -aQ) = 1
    P[4:6] = ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs([a, 1], 4))
    Q[4:6] = gu.g2_mul_gen(curve, [1, r - a])
    P[0] = 0  # product 0 = e(O, Q_0) e(P_1, Q_1) = e(P_1, Q_1)
    Q[7] = 0  # product 3 = e(P_6, Q_6) e(P_7, O) = e(P_6, Q_6)
    P[8] = 0  # product 4 = 1: both pairs hold a point at infinity
    Q[9] = 0
    got, status = backend.pairing_products(curve.cid, P, Q, 2)
    assert not status.any()
    assert (got[2] == _one(curve)).all() and (got[4] == _one(curve)).all()
    assert (got[0] == backend.pairing_product(curve.cid, P[1:2], Q[1:2])).all()
    assert (got[3] == backend.pairing_product(curve.cid, P[6:7], Q[6:7])).all()
    for j in range(5):
        assert (got[j] == backend.pairing_product(curve.cid, P[2 * j:2 * j + 2], Q[2 * j:2 * j + 2])).all(), j


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_a_zero_miller_product_is_a_status_not_a_failure(backend, curve):
    """Q = (1, 0) is not on the twist: doubling it gives (0 : Y : 0), whose tangent line has all three coefficients zero, so the Miller product of its
    product is zero.  zl_pairing_product reports that as ZL_ENOTCURVE; here it is status[1] and a zero row, and the neighbours are untouched."""
    nq = ol.nlq(curve)
    P, Q = (np.array(x[:6]) for x in _pairs(curve))
    Q[3] = 0
    Q[3, 0] = 1  # x = 1 + 0 i, y = 0
    got, status = backend.pairing_products(curve.cid, P, Q, 2)
    assert list(status) == [0, ENOTCURVE, 0]
    assert not got[1].any() and got.shape == (3, 12, nq)
    with pytest.raises(BackendError) as e:
        backend.pairing_product(curve.cid, P[2:4], Q[2:4])
    assert e.value.code == ENOTCURVE
    for j in (0, 2):
        assert (got[j] == backend.pairing_product(curve.cid, P[2 * j:2 * j + 2], Q[2 * j:2 * j + 2])).all(), j


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_empty_batch_empty_products_and_the_pairs_limit(backend, curve):
    P, Q = _pairs(curve)
    got, status = backend.pairing_products(curve.cid, P[:0], Q[:0], 3, count=0)
    assert got.shape[0] == 0 and status.shape[0] == 0
    got, status = backend.pairing_products(curve.cid, P[:0], Q[:0], 0, count=4)
    assert got.shape[0] == 4 and not status.any() and all((g == _one(curve)).all() for g in got)
    # rejected before any work: the arrays are never read
    out = np.zeros((1, 12, ol.nlq(curve)), dtype=np.uint64)
    dummy = np.zeros(1, dtype=np.uint64)
    u64 = lambda a: a.ctypes.data_as(backend.L.zl_pairing_products.argtypes[2])
    rc = backend.L.zl_pairing_products(backend._ctx, curve.cid, u64(dummy), u64(dummy), 1, MAX_PAIRS + 1, u64(out), None)
    assert rc == EINVAL
    with pytest.raises(BackendError) as e:
        backend._check(rc, "zl_pairing_products")
    assert e.value.code == EINVAL


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_chunked_launch_sets_give_the_same_bytes(backend, curve):
    P, Q = _pairs(curve)
    P, Q = P[:33], Q[:33]
    whole, s_whole = backend.pairing_products(curve.cid, P, Q, 3)
    parts, s_parts = _with_chunk(4, lambda: backend.pairing_products(curve.cid, P, Q, 3))  # 11 products: 4 + 4 + 3
    assert whole.tobytes() == parts.tobytes() and s_whole.tobytes() == s_parts.tobytes()
    assert (whole[10] == backend.pairing_product(curve.cid, P[30:33], Q[30:33])).all()
