"""The degenerate Groth16 cases of tests/groth16_degenerate_util.py, pinned on the CPU before any device sees them: for both curves, the shapes `smallest`
(N = 2) and `full16` (N = 16) and two assignments each (the satisfying one and the one with every witness zero), every case

  * holds the relation it is meant to hit (two operands of one tail addition equal, opposite, or one at infinity),
  * gives exponents (A, B, C) that satisfy the Groth16 equation when the assignment satisfies the circuit,
  * and is proved by the C oracle to exactly the points and infinity flags the exponents predict (exponent 0 = all-zero words, flag 1).

Cases per (curve, shape): 2 assignments x 36 = 72 -- nine values of r (eight of the minimum list and the sharded prover's r delta = a0 + Sa), the same nine of s,
both A and B at infinity, r = s = 0, and sixteen values of s aimed at C."""
import numpy as np
import pytest

import groth16_degenerate_util as du
import groth16_util as gu
from oracle_lib import po
from test_gpu_groth16_generic import TD

CURVES = [po.BLS12_381, po.BN254]
CASES_PER_ASSIGNMENT = 36


@pytest.mark.parametrize("which", du.ASSIGNMENTS)
@pytest.mark.parametrize("shape", du.SHAPES)
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_degenerate_cases_hit_their_branch_and_the_oracle_proves_them(curve, shape, which):
    g = du.group(curve, shape, which, TD)
    names = [c.name for c in g.cases]
    assert len(names) == CASES_PER_ASSIGNMENT and set(du.MINIMUM) <= set(names) and set(du.SHARDED) <= set(names)
    if which == "zero_witness":
        assert g.k.L == 0 and not any(g.z[g.cs.n_instance:])
        if shape == "smallest":
            assert g.k.Sa == 0 and g.k.Sb == 0  # no public input: the a / b MSMs are infinity as well
    flags = {"a": 0, "b": 0, "c": 0}
    for c, exp in zip(g.cases, g.expected):
        assert c.holds(), c.name
        assert 0 <= c.r < g.k.p and 0 <= c.s < g.k.p
        A, B, Cx = g.k.proof(c.r, c.s)
        if which == "satisfying":
            assert po.groth16_check_exponents(curve, g.cs, TD, g.pk["ex"], A, B, Cx), c.name
            h_ints = [int(sum(int(w) << (64 * i) for i, w in enumerate(row))) for row in g.h]
            assert po.groth16_prove_exponents(curve, g.cs, TD, g.pk["ex"], h_ints, c.r, c.s) == (A, B, Cx), c.name
        r, s = (np.array([(v >> (64 * i)) & po.MASK64 for i in range(4)], dtype=np.uint64) for v in (c.r, c.s))
        got, _ = gu.oracle_prove(curve, g.arrays, g.zl, g.pk, r, s, threads=1)
        assert (exp[1], exp[3], exp[5]) == (int(A == 0), int(B == 0), int(Cx == 0))
        for i, (x, e) in enumerate(zip(got, exp)):
            assert np.array_equal(np.asarray(x), np.asarray(e)), (c.name, c.what, "a a_inf b b_inf c c_inf".split()[i])
        for key, f in zip("abc", (exp[1], exp[3], exp[5])):
            flags[key] += f
            if f:
                assert not np.asarray(exp["abc".index(key) * 2]).any()
    # A at infinity: r_inf, both_inf; B: s_inf, both_inf; C: c_inf and its two namesakes of the last add
    assert flags["a"] >= 2 and flags["b"] >= 2 and flags["c"] >= 3, flags
    by_name = dict(zip(names, g.expected))
    assert by_name["r_inf"][1] == 1 and by_name["s_inf"][3] == 1 and by_name["c_inf"][5] == 1 and by_name["both_inf"][1] == by_name["both_inf"][3] == 1
