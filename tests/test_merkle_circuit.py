"""The Merkle-membership circuit of the host mirror (R1CS::new_boolean_witness / select, poseidon_merkle in csrc/zl_host.hip) against the independent Python
builder of tests/merkle_circuit_util.py, array for array as tests/test_host_mirror.py does for the chain; its public input against the batched Poseidon entry
points' folds and tree roots; and the host path of zl_poseidon_merkle_assignments against the compilers' assignments.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import groth16_util as gu
import merkle_circuit_util as mu
import oracle_lib as ol
import poseidon_util as pu
from openzl_amd import (BackendError, Circuit, load_library, poseidon_merkle_assignment_elems, poseidon_merkle_assignments_host, poseidon_merkle_build_host,
                        poseidon_merkle_paths_host, poseidon_roots_from_paths_host)

CURVES = pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
DEPTHS = (1, 2, 3, 5)
EINVAL = -1


def indices_of(depth):
    """all-left, all-right and a mixed index (depth 1 has no mixed one)"""
    return sorted({0, (1 << depth) - 1, 0b10110 & ((1 << depth) - 1) or 1})


def case(curve, depth, index):
    """leaf and path values with 0 and r - 1 among them"""
    r = curve.fr.p
    path = pu.random_elems(curve, depth, 100 * depth + index)
    leaf = pu.random_elems(curve, 1, 7 * depth + index)[0]
    if index == 0:
        leaf, path[-1] = 0, r - 1
    elif index == (1 << depth) - 1:
        leaf, path[0] = r - 1, 0
    return leaf, path


@CURVES
@pytest.mark.parametrize("depth", DEPTHS)
def test_compiler_builds_the_python_builders_circuit(curve, depth):
    for index in indices_of(depth):
        leaf, path = case(curve, depth, index)
        c = Circuit.merkle(curve.cid, depth, leaf, index, path)
        w = Circuit.merkle(curve.cid, depth, leaf, index, path, witness_only=True)
        cs = mu.poseidon_merkle_circuit(curve.fr, depth, leaf, index, path)
        try:
            assert c.shape == (cs.n_constraints, cs.n_instance, cs.n_witness) == (237 * depth + 1, 2, 1 + 238 * depth)
            assert c.is_satisfied() and cs.is_satisfied() and w.is_satisfied()
            got, exp = c.arrays(), gu.r1cs_arrays(cs)
            for key in "ABC":
                for g, e in zip(got[key], exp[key]):
                    assert np.array_equal(g, e), (key, index)
            z = ol.ints_to_limbs(cs.assignment(), 4)
            assert np.array_equal(got["assignment"], z)
            wa = w.arrays()
            assert (wa["n_constraints"], wa["n_instance"], wa["n_witness"]) == (0, 2, 1 + 238 * depth)
            assert np.array_equal(wa["assignment"], z)
            # the public input: the plain fold, and the batched entry point's
            root = mu.fold(curve, leaf, index, path)
            assert pu.ints(got["assignment"][1]) == [root]
            folded = poseidon_roots_from_paths_host(curve.cid, pu.limbs([leaf]), [index], pu.limbs(path).reshape(1, depth, 4), depth)
            assert np.array_equal(folded[0], got["assignment"][1])
            # the row writer behind zl_poseidon_merkle_assignments (ctx == NULL)
            rows = poseidon_merkle_assignments_host(curve.cid, pu.limbs([leaf]), [index], pu.limbs(path).reshape(1, depth, 4), depth)
            assert rows.shape == (1, poseidon_merkle_assignment_elems(depth), 4) == (1, 3 + 238 * depth, 4)
            assert np.array_equal(rows[0], z)
        finally:
            c.close()
            w.close()


@CURVES
def test_public_input_is_the_root_of_the_tree_the_paths_come_from(curve):
    """5 leaves at depth 3: leaf 4 has an absent sibling at level 0, leaves 4 and 5's parent an absent one at level 1"""
    n, depth = 5, 3
    leaves = pu.random_elems(curve, n, 55)
    leaves[0] = 0
    lv = pu.limbs(leaves)
    nodes, root = poseidon_merkle_build_host(curve.cid, lv, depth)
    idx = list(range(n))
    paths = poseidon_merkle_paths_host(nodes, n, depth, idx)
    assert not paths[4, 0].any() and not paths[4, 1].any() and paths[4, 2].any()
    rows = poseidon_merkle_assignments_host(curve.cid, lv, idx, paths, depth)
    for i in idx:
        w = Circuit.merkle(curve.cid, depth, leaves[i], i, pu.ints(paths[i]), witness_only=True)
        try:
            z = w.arrays()["assignment"]
        finally:
            w.close()
        assert np.array_equal(z[1], root) and np.array_equal(z[2], lv[i])
        assert np.array_equal(rows[i], z)
    assert np.array_equal(rows[:, 1], np.tile(root, (n, 1)))


@CURVES
def test_python_builder_refuses_a_wrong_path_and_a_bit_that_is_no_bit(curve):
    depth, index = 3, 0b101
    leaf, path = case(curve, depth, index)
    good = mu.poseidon_merkle_circuit(curve.fr, depth, leaf, index, path)
    assert good.is_satisfied()
    root = good.pub[1]
    for level in range(depth):
        changed = list(path)
        changed[level] = (changed[level] + 1) % curve.fr.p
        assert not mu.poseidon_merkle_circuit(curve.fr, depth, leaf, index, changed, root=root).is_satisfied()
    bits = [(index >> j) & 1 for j in range(depth)]
    for level in range(depth):
        bad = list(bits)
        bad[level] = 2
        cs = mu.poseidon_merkle_circuit(curve.fr, depth, leaf, index, path, bits=bad)
        # (1 - 2) * 2 != 0: the Boolean row itself fails, whatever the selects then make of the value
        row = 237 * level
        assert cs.value(cs.A[row]) * cs.value(cs.B[row]) % curve.fr.p != 0 and not cs.C[row].t
        assert not cs.is_satisfied()


@CURVES
def test_error_codes(curve):
    L = load_library()
    r = curve.fr.p
    leaf, path = case(curve, 2, 1)
    lf, pa, idx = pu.limbs([leaf]), pu.limbs(path), np.array([1], dtype=np.uint64)
    out = np.full((1, 3 + 238 * 2, 4), 0xA5, dtype=np.uint64)
    p64 = ol.p64
    assert poseidon_merkle_assignment_elems(0) == 0 and poseidon_merkle_assignment_elems(41) == 0 and poseidon_merkle_assignment_elems(40) == 3 + 238 * 40
    # the circuit hooks
    for fn in (L.zl_circuit_poseidon_merkle, L.zl_circuit_poseidon_merkle_witness):
        h = C.c_void_p()
        big = pu.limbs([1] * 41)
        assert fn(curve.cid, 0, p64(lf), 0, p64(pa), C.byref(h)) == EINVAL
        assert fn(curve.cid, 41, p64(lf), 0, p64(big), C.byref(h)) == EINVAL
        assert fn(curve.cid, 2, p64(lf), 4, p64(pa), C.byref(h)) == EINVAL  # index == 2^depth
        assert fn(curve.cid, 2, None, 1, p64(pa), C.byref(h)) == EINVAL
        assert fn(curve.cid, 2, p64(lf), 1, None, C.byref(h)) == EINVAL
        assert fn(curve.cid, 2, p64(lf), 1, p64(pa), None) == EINVAL
        assert fn(77, 2, p64(lf), 1, p64(pa), C.byref(h)) == EINVAL
        assert not h.value
        assert fn(curve.cid, 2, p64(lf), 3, p64(pa), C.byref(h)) == 0 and h.value
        L.zl_circuit_free(h)
    with pytest.raises(BackendError) as e:
        Circuit.merkle(curve.cid, 2, leaf, 4, path)
    assert e.value.code == EINVAL
    # the assignments, host path
    fn = L.zl_poseidon_merkle_assignments
    assert fn(None, curve.cid, p64(lf), p64(idx), p64(pa), 0, 1, p64(out)) == EINVAL
    assert fn(None, curve.cid, p64(lf), p64(idx), p64(pa), 41, 1, p64(out)) == EINVAL
    assert fn(None, curve.cid, p64(lf), p64(np.array([4], dtype=np.uint64)), p64(pa), 2, 1, p64(out)) == EINVAL
    for bad_leaf, bad_path in ((pu.limbs([r]), pa), (lf, pu.limbs([path[0], r])), (lf, pu.limbs([(1 << 256) - 1, path[1]]))):
        assert fn(None, curve.cid, p64(bad_leaf), p64(idx), p64(bad_path), 2, 1, p64(out.copy())) == EINVAL
    for args in ((None, p64(idx), p64(pa), p64(out)), (p64(lf), None, p64(pa), p64(out)), (p64(lf), p64(idx), None, p64(out)), (p64(lf), p64(idx), p64(pa), None)):
        assert fn(None, curve.cid, args[0], args[1], args[2], 2, 1, args[3]) == EINVAL
    assert fn(None, 77, p64(lf), p64(idx), p64(pa), 2, 1, p64(out)) == EINVAL
    assert (out == 0xA5).all()  # nothing of the refused calls (bar the non-canonical ones, on copies) was written
    assert fn(None, curve.cid, None, None, None, 2, 0, None) == 0  # count == 0: ZL_OK, nothing written
    assert fn(None, curve.cid, p64(lf), p64(idx), p64(pa), 2, 0, p64(out)) == 0 and (out == 0xA5).all()
    assert fn(None, curve.cid, p64(lf), p64(idx), p64(pa), 2, 1, p64(out)) == 0 and (out[0, 0] == [1, 0, 0, 0]).all()
