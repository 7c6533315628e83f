"""Device Miller loops (csrc/zl_pairing_dev.hip) + one host final exponentiation: zl_pairing_product equals the product of single host pairings
(zl_pairing, multiplied in Python Fq12 arithmetic) and the host lock-step multi-pairing, for pair counts around the 64-lane wave and the group sizes; large
products match the bilinear closed form e((sum a_i b_i) G1, G2); infinity, duplicates and inverse pairs behave; every raw per-pair device Miller value,
final-exponentiated on the host, is that pair's pairing."""
import numpy as np
import pytest

import groth16_util as gu
import oracle_lib as ol
from oracle_lib import po
from openzl_amd import ZL_G1, ZL_G2, pairing, pairing_product
from openzl_amd.backend import hook_final_exp, hook_miller_dev, hook_pairing_product

CURVES = [po.BLS12_381, po.BN254]
ONE = [1] + [0] * 11


def _pairs(curve, n, seed):
    a = ol.random_scalars(curve, n, seed)
    b = ol.random_scalars(curve, n, seed + 1)
    return ol.oracle_g1_mul_gen(curve, a), gu.g2_mul_gen(curve, ol.limbs_to_ints(b))


def _product_of_singles(curve, P, Q):
    ctx = po.Fq12Ctx(curve)
    acc = ONE
    for i in range(P.shape[0]):
        acc = ctx.mul(acc, ol.limbs_to_ints(pairing(curve.cid, P[i], Q[i])))
    return acc


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_pairing_product_small_counts(backend, curve):
    P, Q = _pairs(curve, 65, 11)
    for n in (1, 2, 3, 63, 64, 65):
        got = backend.pairing_product(curve.cid, P[:n], Q[:n])
        assert ol.limbs_to_ints(got) == _product_of_singles(curve, P[:n], Q[:n]), n
        if n <= 64:
            assert (got == hook_pairing_product(curve.cid, P[:n], Q[:n])).all(), n
    assert ol.limbs_to_ints(pairing_product(backend, curve.cid, P[:0], Q[:0])) == ONE


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("n", [1000, 4097])
def test_pairing_product_large_counts_match_bilinearity(backend, curve, n):
    a = ol.random_scalars(curve, n, 21)
    b = ol.random_scalars(curve, n, 22)
    h1 = backend.bases_generate(curve.cid, a, group=ZL_G1)
    h2 = backend.bases_generate(curve.cid, b, group=ZL_G2)
    try:
        P, Q = backend.bases_download(h1), backend.bases_download(h2)
    finally:
        backend.bases_free(h1)
        backend.bases_free(h2)
    r = curve.fr.p
    s = sum(x * y for x, y in zip(ol.limbs_to_ints(a), ol.limbs_to_ints(b))) % r
    exp = pairing(curve.cid, ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs([s], 4))[0], gu.g2_mul_gen(curve, [1])[0])
    assert (backend.pairing_product(curve.cid, P, Q) == exp).all()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_pairing_product_edge_pairs(backend, curve):
    r = curve.fr.p
    a = 0x5EED5EED5EED
    P = ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs([1, r - 1, 7, a, 1], 4))
    Q = gu.g2_mul_gen(curve, [r - 1, 1, 9, 1, r - a])
    # scalars 1 and r - 1: e(G1, -G2) e(-G1, G2) = e(G1, G2)^-2
    got = backend.pairing_product(curve.cid, P[:2], Q[:2])
    assert ol.limbs_to_ints(got) == _product_of_singles(curve, P[:2], Q[:2])
    # P or Q at infinity contributes 1
    Pz, Qz = P[2:3].copy(), Q[2:3].copy()
    Pz[:] = 0
    assert ol.limbs_to_ints(backend.pairing_product(curve.cid, Pz, Q[2:3])) == ONE
    Qz[:] = 0
    assert ol.limbs_to_ints(backend.pairing_product(curve.cid, P[2:3], Qz)) == ONE
    mixed_P = np.concatenate([P[2:3], Pz, P[2:3]])
    mixed_Q = np.concatenate([Q[2:3], Q[2:3], Qz])
    assert (backend.pairing_product(curve.cid, mixed_P, mixed_Q) == pairing(curve.cid, P[2], Q[2])).all()
    # a duplicated pair squares its pairing
    ctx = po.Fq12Ctx(curve)
    e = ol.limbs_to_ints(pairing(curve.cid, P[2], Q[2]))
    assert ol.limbs_to_ints(backend.pairing_product(curve.cid, P[[2, 2]], Q[[2, 2]])) == ctx.mul(e, e)
    # e(aP, Q) e(P, -aQ) = 1
    assert ol.limbs_to_ints(backend.pairing_product(curve.cid, P[3:5], Q[3:5])) == ONE


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_raw_device_miller_values_exponentiate_to_the_host_pairing(backend, curve):
    P, Q = _pairs(curve, 70, 31)
    P[5] = 0  # infinity: a Miller value of 1
    raw = hook_miller_dev(backend, curve.cid, P, Q)
    assert ol.limbs_to_ints(raw[5]) == ONE
    for i in range(P.shape[0]):
        assert (hook_final_exp(curve.cid, raw[i]) == pairing(curve.cid, P[i], Q[i])).all(), f"pair {i}"
