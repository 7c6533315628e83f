"""Groth16 on generic R1CS circuits (tests/r1cs_gen.py), CPU side: the C oracle's quotient h equals the Python restatement of the
witness map on every shape of the table, satisfied circuits give an h of degree < N - 1 and oracle proofs that satisfy the Groth16
equation in the exponent, unsatisfied ones a full-degree h.  The shapes are checked to hold what they are there for (empty rows,
rows of > 64 terms, one-term A rows, long C rows, CSR entries an LC cannot express), so that the device tests over the same table
cover those paths."""
import numpy as np
import pytest

import groth16_util as gu
import oracle_lib as ol
import r1cs_gen as rg
from oracle_lib import po

CURVES = [po.BLS12_381, po.BN254]
TD = po.Groth16Trapdoor(alpha=0x5151_2323_7878, beta=0x2468_ACE0_1357, gamma=0x9BDF_1111, delta=0x7777_1234_4321, tau=0xABCD_EF01_2345_6789)
R_, S_ = 0x3141_5926_5358_9793_2384, 0x2718_2818_2845_9045_2353


def _infinity_key(curve) -> dict:
    """h does not depend on the key: points at infinity keep the oracle's MSMs trivial"""
    nq = ol.nlq(curve)
    g1 = lambda n: np.zeros((n, 2 * nq), dtype=np.uint64)
    return {"a_query": g1(rg.KEY_NV), "b_g1_query": g1(rg.KEY_NV), "h_query": g1(rg.KEY_NH), "l_query": g1(rg.KEY_NW),
            "b_g2_query": np.zeros((rg.KEY_NV, 4 * nq), dtype=np.uint64), "alpha_g1": g1(1)[0], "beta_g1": g1(1)[0], "delta_g1": g1(1)[0],
            "beta_g2": np.zeros(4 * nq, dtype=np.uint64), "delta_g2": np.zeros(4 * nq, dtype=np.uint64)}


def _scalars(curve):
    return ol.ints_to_limbs([R_ % curve.fr.p, S_ % curve.fr.p], 4)


@pytest.mark.parametrize("name", list(rg.SHAPES))
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_generic_witness_map_oracle_matches_python(curve, name):
    cs, arrays = rg.shape_case(curve, name)
    spec = rg.SHAPES[name]
    assert (cs.n_constraints, cs.n_instance, cs.n_witness) == (spec["n_constraints"], spec["n_instance"], spec["n_witness"])
    n = 1 << cs.domain_log()
    r, s = _scalars(curve)
    z = ol.ints_to_limbs(cs.assignment(), 4)
    _, h = gu.oracle_prove(curve, arrays, z, _infinity_key(curve), r, s, threads=8, want_h=n)
    h_py = po.qap_witness_map(curve, cs)
    assert ol.limbs_to_ints(h) == h_py
    if spec.get("satisfied", True):
        assert cs.is_satisfied() and h_py[-1] == 0
    else:
        assert not cs.is_satisfied() and h_py[-1] != 0  # a full-degree quotient: the case is not degenerate


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_generic_shapes_hold_what_they_test(curve):
    """each shape of the table has the property that its device test is there for"""
    shape = {name: rg.shape_case(curve, name) for name in rg.SHAPES}

    def row_lengths(arrays, key):
        return np.diff(arrays[key][0].astype(np.int64))

    def domain(cs):
        return 1 << cs.domain_log()

    cs, _ = shape["smallest"]
    assert domain(cs) == 2
    cs, _ = shape["full16"]
    assert cs.n_constraints + cs.n_instance == domain(cs) == 16
    cs, _ = shape["full17"]
    assert cs.n_constraints + cs.n_instance == 17 and domain(cs) == 32
    cs, arrays = shape["many_publics"]
    assert cs.n_instance > cs.n_constraints and row_lengths(arrays, "A").mean() >= 4  # eight-lane A with a tail longer than the rows
    cs, _ = shape["no_witness"]
    assert cs.n_witness == 0
    for name in ("sparse_a", "unsat_sparse_a"):
        cs, arrays = shape[name]
        assert row_lengths(arrays, "A").max() == 1 and (row_lengths(arrays, "C") == 0).any()  # boolean rows: one-lane A, empty C rows
    cs, arrays = shape["long_c"]
    assert row_lengths(arrays, "C").min() >= 4
    for name in ("mixed", "unsat_mixed"):
        cs, arrays = shape[name]
        lens = row_lengths(arrays, "A") + row_lengths(arrays, "B") + row_lengths(arrays, "C")
        assert (lens == 0).any() and max(row_lengths(arrays, "A").max(), row_lengths(arrays, "B").max()) > 64
    # the CSR edges: an explicit zero, a row whose columns are not ascending, a column twice in one row -- in every matrix
    cs, arrays = shape["edges"]
    for key in "ABC":
        ptr, col, val = arrays[key]
        rows = [col[ptr[i]:ptr[i + 1]] for i in range(len(ptr) - 1)]
        assert (~val.any(axis=1)).any()
        assert any((np.diff(rw.astype(np.int64)) < 0).any() for rw in rows)
        assert any(len(set(rw.tolist())) < len(rw) for rw in rows)
    # every value the generator weights on shows up in the assignments and coefficients of the table
    vals = set()
    coefs = set()
    for cs, _ in shape.values():
        vals.update(cs.assignment()[1:])
        for m in (cs.A, cs.B, cs.C):
            for row in m:
                coefs.update(row.t.values())
    p = curve.fr.p
    assert {0, 1, p - 1} <= vals and {1, p - 1} <= coefs


@pytest.mark.parametrize("name", ["smallest", "many_publics"])
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_generic_oracle_proof_satisfies_groth16_equation(curve, name):
    """the oracle's proof of a generic circuit is the group element that the exponents of a trapdoor setup predict"""
    cs, arrays = rg.shape_case(curve, name)
    pk = gu.setup_with_trapdoor(curve, cs, TD)
    n = 1 << cs.domain_log()
    r, s = _scalars(curve)
    (a, ai, b, bi, c, ci), h = gu.oracle_prove(curve, arrays, ol.ints_to_limbs(cs.assignment(), 4), pk, r, s, threads=8, want_h=n)
    h_ints = ol.limbs_to_ints(h)
    assert h_ints == po.qap_witness_map(curve, cs) and h_ints[-1] == 0
    A, B, Cx = po.groth16_prove_exponents(curve, cs, TD, pk["ex"], h_ints, R_ % curve.fr.p, S_ % curve.fr.p)
    assert po.groth16_check_exponents(curve, cs, TD, pk["ex"], A, B, Cx)
    assert not (ai or bi or ci)
    assert (a == ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs([A], 4))[0]).all()
    assert (b == gu.g2_mul_gen(curve, [B])[0]).all()
    assert (c == ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs([Cx], 4))[0]).all()
