"""The two arity-general circuits of the host mirror (poseidon::hash<FrP, W> in csrc/zl_host.h, poseidon_arity in csrc/zl_host.hip) against the independent
Python builder of tests/arity_circuit_util.py, array for array, at arity 2..5 on both curves: CSR matrices and assignment of the full compiler, the assignment
of the witness-only compiler, satisfaction of the exported rows (and its loss when the public input or one record is altered), the arity-2 hash circuit
against the one-link chain, and every ZL_EINVAL.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import arity_circuit_util as au
import groth16_util as gu
import oracle_lib as ol
import poseidon_arity_util as pa
import poseidon_util as pu
from openzl_amd import BackendError, Circuit, load_library

CURVES = pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
ARITIES = pytest.mark.parametrize("arity", pa.ARITIES)
EINVAL = -1


def csr_satisfied(arrays, z, p) -> bool:
    """A z * B z == C z row by row over exported CSR arrays and an assignment of Python integers"""
    prod = []
    for key in "ABC":
        ptr, col, val = arrays[key]
        vals = ol.limbs_to_ints(val) if len(col) else []
        prod.append([sum(vals[t] * z[int(col[t])] for t in range(int(ptr[i]), int(ptr[i + 1]))) % p for i in range(arrays["n_constraints"])])
    return all(a * b % p == c for a, b, c in zip(*prod))


def same_arrays(got, exp):
    return all(np.array_equal(g, e) for key in "ABC" for g, e in zip(got[key], exp[key]))


def hash_inputs(curve, arity):
    """random inputs, then 0 and r - 1 in every position"""
    r = curve.fr.p
    base = pu.random_elems(curve, arity, 30 + arity)
    cases = [list(base)]
    for pos in range(arity):
        for v in (0, r - 1):
            x = list(base)
            x[pos] = v
            cases.append(x)
    return cases


@CURVES
@ARITIES
def test_hash_compiler_builds_the_python_builders_circuit(curve, arity):
    p = curve.fr.p
    for n, x in enumerate(hash_inputs(curve, arity)):
        w = Circuit.poseidon_hash(curve.cid, x, witness_only=True)
        cs = au.poseidon_hash_circuit(curve.fr, x)
        z = ol.ints_to_limbs(cs.assignment(), 4)
        try:
            assert cs.is_satisfied() and w.is_satisfied()
            wa = w.arrays()
            assert (wa["n_constraints"], wa["n_instance"], wa["n_witness"]) == (0, 2, arity + 3 * au.SBOXES[arity])
            assert np.array_equal(wa["assignment"], z), n
            assert pu.ints(z[1]) == [pa.hash(curve, x)]
        finally:
            w.close()
        # The matrices do not depend on the values (the gadget folds only the constant lane), so the full compiler -- whose symbolic synthesis is the slow part --
        # runs on three cases; every case goes through the witness-only compiler above.  The tamper checks below evaluate the C compiler's EXPORTED rows in
        # Python: the library's own is_satisfied has no hook to alter an assignment, and the exported arrays are what a prover is handed.
        if n not in (0, 1, 2 * arity):  # the full compiler on the random case, the first 0 and the last r - 1
            continue
        c = Circuit.poseidon_hash(curve.cid, x)
        try:
            assert c.shape == (cs.n_constraints, cs.n_instance, cs.n_witness) == au.hash_shape(arity) == (3 * au.SBOXES[arity] + 1, 2, arity + 3 * au.SBOXES[arity])
            assert c.is_satisfied()
            got = c.arrays()
            assert same_arrays(got, gu.r1cs_arrays(cs)), n
            assert np.array_equal(got["assignment"], z), n
            if n == 0:
                zi = cs.assignment()
                assert csr_satisfied(got, zi, p)
                bad = list(zi)
                bad[1] = (bad[1] + 1) % p  # the public input
                assert not csr_satisfied(got, bad, p)
                for at in (2 + arity, 2 + arity + 3 * (arity + 1), len(zi) - 1):  # the first record, one of round 1, the last
                    bad = list(zi)
                    bad[at] = (bad[at] + 1) % p
                    assert not csr_satisfied(got, bad, p), at
                assert not au.poseidon_hash_circuit(curve.fr, x, digest=(zi[1] + 1) % p).is_satisfied()
        finally:
            c.close()


@CURVES
def test_arity_two_hash_circuit_is_the_one_link_chain(curve):
    x0, x1 = pu.random_elems(curve, 2, 77)
    h = Circuit.poseidon_hash(curve.cid, [x0, x1])
    c = Circuit(curve.cid, 1, x0, x1)
    hw = Circuit.poseidon_hash(curve.cid, [x0, x1], witness_only=True)
    cw = Circuit(curve.cid, 1, x0, x1, witness_only=True)
    try:
        assert h.shape == c.shape == (235, 2, 236)
        a, b = h.arrays(), c.arrays()
        assert same_arrays(a, b) and np.array_equal(a["assignment"], b["assignment"])
        assert np.array_equal(hw.arrays()["assignment"], cw.arrays()["assignment"]) and np.array_equal(hw.arrays()["assignment"], a["assignment"])
    finally:
        for x in (h, c, hw, cw):
            x.close()


def leaf_cases(curve, arity):
    """(depth, index, preimage, path): depth 1 and 2 at index 0 and 2^d - 1, a zero sibling, and 0 and r - 1 in every preimage position"""
    r = curve.fr.p
    base = pu.random_elems(curve, arity, 50 + arity)
    out = []
    for depth in (1, 2):
        for index in (0, (1 << depth) - 1):
            path = pu.random_elems(curve, depth, 60 + 10 * depth + index)
            if index == 0:
                path[depth - 1] = 0
            out.append((depth, index, list(base), path))
    path = pu.random_elems(curve, 2, 90)
    for pos in range(arity):
        for v in (0, r - 1):
            x = list(base)
            x[pos] = v
            out.append((2, 1 + (pos & 1), x, path))
    return out


@CURVES
@ARITIES
def test_leaf_membership_compiler_builds_the_python_builders_circuit(curve, arity):
    p = curve.fr.p
    for n, (depth, index, pre, path) in enumerate(leaf_cases(curve, arity)):
        w = Circuit.merkle_leaf(curve.cid, depth, pre, index, path, witness_only=True)
        cs = au.poseidon_merkle_leaf_circuit(curve.fr, depth, pre, index, path)
        z = ol.ints_to_limbs(cs.assignment(), 4)
        try:
            assert cs.is_satisfied() and w.is_satisfied()
            wa = w.arrays()
            assert (wa["n_constraints"], wa["n_instance"], wa["n_witness"]) == (0, 2, au.leaf_shape(arity, depth)[2])
            assert np.array_equal(wa["assignment"], z), n
            assert pu.ints(z[1]) == [au.leaf_root(curve, pre, index, path)]
        finally:
            w.close()
        # (as above: the rows depend on arity, depth and nothing else -- Boolean and select always allocate -- so five cases see the full compiler)
        if n >= 5:  # the full compiler on the four (depth, index) cases and the first edge preimage
            continue
        c = Circuit.merkle_leaf(curve.cid, depth, pre, index, path)
        try:
            s3 = 3 * au.SBOXES[arity]
            assert c.shape == (cs.n_constraints, cs.n_instance, cs.n_witness) == (s3 + 237 * depth + 1, 2, arity + s3 + 238 * depth)
            assert c.is_satisfied()
            got = c.arrays()
            assert same_arrays(got, gu.r1cs_arrays(cs)), n
            assert np.array_equal(got["assignment"], z), n
            if n == 3:  # depth 2, index 3
                zi = cs.assignment()
                assert csr_satisfied(got, zi, p)
                level1 = 2 + arity + s3 + 238
                for at in (1, 2, 2 + arity, 2 + arity + s3 - 1, level1, level1 + 1, level1 + 2, level1 + 4, len(zi) - 1):
                    bad = list(zi)  # the root, a preimage element, records of the leaf hash, a sibling, its bit, a select, records of a level
                    bad[at] = (bad[at] + 1) % p
                    assert not csr_satisfied(got, bad, p), at
        finally:
            c.close()


@CURVES
def test_error_codes(curve):
    L = load_library()
    r = curve.fr.p
    p64 = ol.p64
    x = pu.limbs(pu.random_elems(curve, 5, 5))
    pa2 = pu.limbs(pu.random_elems(curve, 2, 6))
    big = pu.limbs([1] * 41)
    for fn in (L.zl_circuit_poseidon_hash, L.zl_circuit_poseidon_hash_witness):
        h = C.c_void_p()
        for arity in (0, 1, 6):
            assert fn(curve.cid, arity, p64(x), C.byref(h)) == EINVAL
        assert fn(curve.cid, 3, None, C.byref(h)) == EINVAL
        assert fn(curve.cid, 3, p64(x), None) == EINVAL
        assert fn(77, 3, p64(x), C.byref(h)) == EINVAL
        for pos in range(3):
            for v in (r, (1 << 256) - 1):
                bad = x.copy()
                bad[pos] = pu.limbs([v])[0]
                assert fn(curve.cid, 3, p64(bad), C.byref(h)) == EINVAL
        assert not h.value
        assert fn(curve.cid, 3, p64(x), C.byref(h)) == 0 and h.value
        L.zl_circuit_free(h)
    for fn in (L.zl_circuit_poseidon_merkle_leaf, L.zl_circuit_poseidon_merkle_leaf_witness):
        h = C.c_void_p()
        for arity in (0, 1, 6):
            assert fn(curve.cid, arity, 2, p64(x), 1, p64(pa2), C.byref(h)) == EINVAL
        assert fn(curve.cid, 4, 0, p64(x), 0, p64(pa2), C.byref(h)) == EINVAL
        assert fn(curve.cid, 4, 41, p64(x), 0, p64(big), C.byref(h)) == EINVAL
        assert fn(curve.cid, 4, 2, p64(x), 4, p64(pa2), C.byref(h)) == EINVAL  # index == 2^depth
        assert fn(curve.cid, 4, 2, None, 1, p64(pa2), C.byref(h)) == EINVAL
        assert fn(curve.cid, 4, 2, p64(x), 1, None, C.byref(h)) == EINVAL
        assert fn(curve.cid, 4, 2, p64(x), 1, p64(pa2), None) == EINVAL
        assert fn(77, 4, 2, p64(x), 1, p64(pa2), C.byref(h)) == EINVAL
        bad = x.copy()
        bad[3] = pu.limbs([r])[0]
        assert fn(curve.cid, 4, 2, p64(bad), 1, p64(pa2), C.byref(h)) == EINVAL  # a preimage element at r
        bad_pa = pa2.copy()
        bad_pa[1] = pu.limbs([r])[0]
        assert fn(curve.cid, 4, 2, p64(x), 1, p64(bad_pa), C.byref(h)) == EINVAL  # a sibling at r
        assert not h.value
        assert fn(curve.cid, 4, 2, p64(x), 3, p64(pa2), C.byref(h)) == 0 and h.value
        L.zl_circuit_free(h)
        bad[3] = x[3]
        bad[4] = pu.limbs([r])[0]  # element 4 is not part of an arity-4 preimage
        h = C.c_void_p()
        assert fn(curve.cid, 4, 2, p64(bad), 3, p64(pa2), C.byref(h)) == 0
        L.zl_circuit_free(h)
    xs, path = pu.ints(x), pu.ints(pa2)
    for make in (lambda: Circuit.poseidon_hash(curve.cid, xs[:1]), lambda: Circuit.poseidon_hash(curve.cid, xs + [1]), lambda: Circuit.poseidon_hash(curve.cid, [1, r]),
                 lambda: Circuit.merkle_leaf(curve.cid, 2, xs[:3], 4, path), lambda: Circuit.merkle_leaf(curve.cid, 3, xs[:3], 1, path),
                 lambda: Circuit.merkle_leaf(curve.cid, 2, xs[:3], 1, [path[0], r])):
        with pytest.raises(BackendError) as e:
            make()
        assert e.value.code == EINVAL
