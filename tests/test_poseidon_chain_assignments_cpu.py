"""zl_poseidon_chain_assignments on its host path (ctx == NULL: the host mirror's permute_native_record over the host pool): the complete assignment of the
Poseidon-chain circuit per chain -- 1, h_k, x0, x1, then x^2, x^4, x^5 of every S-box the circuit allocates -- must equal, word for word, what the witness-only
compiler AND the full compiler export for the same inputs.  k = 1: link 1 takes plain variables; k = 2, 3: later links take the previous digest; k = 3: the
full compiler's replicate_rows values start.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import poseidon_util as pu
from oracle_lib import po
from openzl_amd import Circuit, load_library, poseidon_chain_assignment_elems, poseidon_chain_assignments_host, poseidon_chain_host
from openzl_amd import backend as zb

HERE = os.path.dirname(os.path.abspath(__file__))
FX = json.load(open(os.path.join(HERE, "golden", "ref_poseidon_fixtures.json")))
CURVES = pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
OK, EINVAL = 0, -1


def inputs(curve):
    """(0, 0), (r - 1, r - 1), (1, 2) and three random pairs"""
    r = curve.fr.p
    rnd = pu.random_elems(curve, 6, 0xC4A1)
    return [0, r - 1, 1] + rnd[:3], [0, r - 1, 2] + rnd[3:]


@CURVES
@pytest.mark.parametrize("k", [1, 2, 3])
def test_rows_are_the_compilers_assignments(curve, k):
    x0, x1 = inputs(curve)
    got = poseidon_chain_assignments_host(curve.cid, pu.limbs(x0), pu.limbs(x1), k)
    nv = 4 + 234 * k
    assert got.shape == (len(x0), nv, 4)
    digests = poseidon_chain_host(curve.cid, pu.limbs(x0), pu.limbs(x1), k)
    for i, (a, b) in enumerate(zip(x0, x1)):
        for witness_only in (True, False):
            c = Circuit(curve.cid, k, a, b, witness_only=witness_only)
            try:
                if not witness_only:
                    assert c.shape == (234 * k + 1, 2, 2 + 234 * k) and c.is_satisfied()
                exp = c.arrays()["assignment"]
            finally:
                c.close()
            assert exp.shape == (nv, 4)
            assert got[i].tobytes() == exp.tobytes(), (i, witness_only)
        assert pu.ints(got[i, 0]) == [1] and pu.ints(got[i, 2]) == [a] and pu.ints(got[i, 3]) == [b]
        assert np.array_equal(got[i, 1], digests[i])


def test_h_1_of_1_2_is_the_reference_digest():
    got = poseidon_chain_assignments_host(po.BLS12_381.cid, pu.limbs([1]), pu.limbs([2]), 1)
    assert str(pu.ints(got[0, 1])[0]) == FX["permutation_width3"]["output"][0]


def test_the_first_records_are_the_s_boxes_of_round_0():
    """lane 0 of round 0 is not recorded: the row goes on with x^2, x^4, x^5 of lane 1 (x0 + key 1), then of lane 2 (x1 + key 2)"""
    curve = po.BLS12_381
    p = curve.fr.p
    keys, _ = pu.constants(curve.name)
    x0, x1 = 5, 7
    row = pu.ints(poseidon_chain_assignments_host(curve.cid, pu.limbs([x0]), pu.limbs([x1]), 1)[0])
    exp = []
    for v in ((x0 + keys[1]) % p, (x1 + keys[2]) % p):
        exp += [pow(v, 2, p), pow(v, 4, p), pow(v, 5, p)]
    assert row[4:10] == exp


def test_elems():
    assert [poseidon_chain_assignment_elems(k) for k in (1, 2, 3, 0)] == [238, 472, 706, 0]
    assert poseidon_chain_assignment_elems(64) == 14980
    top = ((1 << 31) - 1 - 4) // 234  # the largest k whose variable count fits 31 bits
    assert poseidon_chain_assignment_elems(top) == 4 + 234 * top and poseidon_chain_assignment_elems(top + 1) == 0
    assert poseidon_chain_assignment_elems((1 << 32) - 1) == 0


@CURVES
def test_errors_and_empty_batch(curve):
    L = load_library()
    x0, x1 = pu.limbs([1, 2]), pu.limbs([3, 4])
    out = np.full((2, 238, 4), 0xA5, dtype=np.uint64)
    call = lambda a, b, k, n, o: L.zl_poseidon_chain_assignments(None, curve.cid, a, b, k, n, o)  # noqa: E731
    assert call(zb._p64(x0), zb._p64(x1), 0, 2, zb._p64(out)) == EINVAL
    assert call(None, zb._p64(x1), 1, 2, zb._p64(out)) == EINVAL
    assert call(zb._p64(x0), None, 1, 2, zb._p64(out)) == EINVAL
    assert call(zb._p64(x0), zb._p64(x1), 1, 2, None) == EINVAL
    assert L.zl_poseidon_chain_assignments(None, 99, zb._p64(x0), zb._p64(x1), 1, 2, zb._p64(out)) == EINVAL
    assert call(zb._p64(x0), zb._p64(x1), 1, 0, zb._p64(out)) == OK
    assert call(None, None, 1, 0, None) == OK
    assert (out == 0xA5).all()  # nothing was written by any call above
    for at in (0, 1):
        bad = [pu.limbs([1, 2]), pu.limbs([3, 4])]
        bad[at] = pu.limbs([1, curve.fr.p])
        assert call(zb._p64(bad[0]), zb._p64(bad[1]), 1, 2, zb._p64(out.copy())) == EINVAL
    with pytest.raises(zb.BackendError) as e:
        poseidon_chain_assignments_host(curve.cid, pu.limbs([curve.fr.p]), pu.limbs([1]), 2)
    assert e.value.code == EINVAL
    # a row that would not fit the staging budget (64 + 32 (4 + 234 k) bytes > 256 MiB) is refused before any work, on the host path too
    assert poseidon_chain_assignment_elems(35849) != 0
    assert call(zb._p64(x0), zb._p64(x1), 35849, 1, zb._p64(out)) == EINVAL
    assert call(None, None, 35849, 0, None) == EINVAL and call(None, None, 35848, 0, None) == OK
    assert (out == 0xA5).all()
    # the device form has no host path: a null ctx is refused
    assert L.zl_poseidon_chain_assignments_dev(None, curve.cid, C.c_void_p(16), C.c_void_p(16), 1, 1, C.c_void_p(16), 238) == EINVAL
    assert call(zb._p64(x0), zb._p64(x1), 1, 2, zb._p64(out)) == OK and pu.ints(out[:, 0]) == [1, 1]
