"""The inverse in Fq12 by a chain of norms (csrc/zl_fq12_inv.h; the device final exponentiation k_pd_fexp takes the same steps, one coefficient per lane), run on
the host through zl_test_fq12_inverse and compared with the oracle's polynomial inverse po.Fq12Ctx.inv: random elements, elements with one non-zero
coefficient, elements of the subfields Fq and Fq[w^6], one; zero reports singular; the chain's zeta is a primitive cube root of unity in Fq."""
import random

import pytest

import oracle_lib as ol
from oracle_lib import po
from openzl_amd.backend import hook_fq12_inverse, hook_fq12_zeta

CURVES = [po.BLS12_381, po.BN254]


def _inv(curve, f):
    out, singular = hook_fq12_inverse(curve.cid, ol.ints_to_limbs(f, ol.nlq(curve)))
    return ol.limbs_to_ints(out), singular


def _cases(curve):
    q = curve.fq.p
    rng = random.Random(0xF12 + curve.cid)
    rnd = lambda: rng.randrange(1, q)
    cases = [("random", [rng.randrange(q) for _ in range(12)]) for _ in range(6)]
    cases += [(f"w^{k}", [rnd() if i == k else 0 for i in range(12)]) for k in range(12)]
    cases += [("w^k, coefficient q - 1", [q - 1 if i == 7 else 0 for i in range(12)])]
    cases += [("Fq", [rnd()] + [0] * 11), ("Fq: 2", [2] + [0] * 11), ("Fq: q - 1", [q - 1] + [0] * 11)]
    cases += [("Fq[w^6]", [rnd() if i in (0, 6) else 0 for i in range(12)]) for _ in range(3)]
    cases += [("even coefficients only", [rnd() if i % 2 == 0 else 0 for i in range(12)])]
    cases += [("one", [1] + [0] * 11)]
    return cases


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_chain_equals_the_oracle_inverse(curve):
    ctx = po.Fq12Ctx(curve)
    for what, f in _cases(curve):
        got, singular = _inv(curve, f)
        assert not singular, what
        assert got == ctx.inv(f), what
        assert ctx.mul(got, f) == [1] + [0] * 11, what


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_zero_is_singular_with_a_zero_result(curve):
    got, singular = _inv(curve, [0] * 12)
    assert singular and got == [0] * 12


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_zeta_is_a_primitive_cube_root_of_unity(curve):
    q = curve.fq.p
    (zeta,) = ol.limbs_to_ints(hook_fq12_zeta(curve.cid)[None])
    assert 1 < zeta < q and pow(zeta, 3, q) == 1
    assert (zeta * zeta + zeta + 1) % q == 0
