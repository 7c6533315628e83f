"""The host mirror behind zl_poseidon_hash_assignments and zl_poseidon_merkle_leaf_assignments (ctx == NULL: host_hash_assignments / host_leaf_assignments in
csrc/zl_poseidon_dev.hip) against the assignments both host compilers export, at arity 2..5 on both curves; the row sizes; the arity-2 hash rows against
the one-link chain rows; and the argument errors.  The member form (zl_poseidon_merkle_leaf_member_assignments_dev) has no host mirror -- it takes device
pointers only -- so its digest mismatch is exercised in tests/test_gpu_poseidon_arity_assignments.py.  No GPU."""
import numpy as np
import pytest

import arity_circuit_util as au
import oracle_lib as ol
import poseidon_arity_util as pa
import poseidon_util as pu
from openzl_amd import (Circuit, load_library, poseidon_chain_assignments_host, poseidon_hash_assignment_elems, poseidon_hash_assignments_host, poseidon_hash_host,
                        poseidon_merkle_leaf_assignment_elems, poseidon_merkle_leaf_assignments_host)

CURVES = pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
ARITIES = pytest.mark.parametrize("arity", pa.ARITIES)
EINVAL = -1


def witness_assignment(make):
    w = make()
    try:
        return w.arrays()["assignment"]
    finally:
        w.close()


def test_row_sizes():
    for a, s in au.SBOXES.items():
        assert poseidon_hash_assignment_elems(a) == 2 + a + 3 * s
        for d in (1, 7, 40):
            assert poseidon_merkle_leaf_assignment_elems(a, d) == 2 + a + 3 * s + 238 * d
        assert poseidon_merkle_leaf_assignment_elems(a, 0) == 0 and poseidon_merkle_leaf_assignment_elems(a, 41) == 0
    assert [poseidon_hash_assignment_elems(a) for a in (2, 3, 4, 5)] == [238, 263, 291, 316]
    for a in (0, 1, 6):
        assert poseidon_hash_assignment_elems(a) == 0 and poseidon_merkle_leaf_assignment_elems(a, 3) == 0


@CURVES
@ARITIES
def test_hash_rows_equal_the_compilers_assignments(curve, arity):
    r = curve.fr.p
    xs = [pu.random_elems(curve, arity, 200 + 7 * j + arity) for j in range(40)]  # more than one block of the host pool
    for pos in range(arity):
        xs[2 * pos][pos], xs[2 * pos + 1][pos] = 0, r - 1
    v = pu.limbs([e for x in xs for e in x]).reshape(len(xs), arity, 4)
    rows = poseidon_hash_assignments_host(curve.cid, v)
    assert rows.shape == (len(xs), poseidon_hash_assignment_elems(arity), 4)
    assert np.array_equal(rows[:, 0], np.tile(np.array([1, 0, 0, 0], dtype=np.uint64), (len(xs), 1)))
    assert np.array_equal(rows[:, 1], poseidon_hash_host(curve.cid, v))
    assert np.array_equal(rows[:, 2:2 + arity], v)
    for j in list(range(2 * arity)) + [39]:
        assert np.array_equal(rows[j], witness_assignment(lambda: Circuit.poseidon_hash(curve.cid, xs[j], witness_only=True))), j
    full = Circuit.poseidon_hash(curve.cid, xs[1])
    try:
        assert np.array_equal(rows[1], full.arrays()["assignment"])
    finally:
        full.close()
    assert np.array_equal(rows[5], ol.ints_to_limbs(au.poseidon_hash_circuit(curve.fr, xs[5]).assignment(), 4))
    assert poseidon_hash_assignments_host(curve.cid, v[:0]).shape == (0, poseidon_hash_assignment_elems(arity), 4)


@CURVES
def test_arity_two_hash_rows_are_the_one_link_chain_rows(curve):
    xs = pu.limbs(pu.random_elems(curve, 10, 9)).reshape(5, 2, 4)
    a = poseidon_hash_assignments_host(curve.cid, xs)
    b = poseidon_chain_assignments_host(curve.cid, np.ascontiguousarray(xs[:, 0]), np.ascontiguousarray(xs[:, 1]), 1)
    assert a.tobytes() == b.tobytes()


@CURVES
@ARITIES
@pytest.mark.parametrize("depth", [1, 3])
def test_leaf_membership_rows_equal_the_compilers_assignments(curve, arity, depth):
    r = curve.fr.p
    count = 2 * arity + 4
    pre = [pu.random_elems(curve, arity, 300 + 11 * j + arity) for j in range(count)]
    paths = [pu.random_elems(curve, depth, 400 + 13 * j + depth) for j in range(count)]
    idx = [(3 * j + 1) % (1 << depth) for j in range(count)]
    for pos in range(arity):
        pre[2 * pos][pos], pre[2 * pos + 1][pos] = 0, r - 1
    idx[0], idx[1] = 0, (1 << depth) - 1
    paths[2][0] = 0
    paths[3][depth - 1] = 0
    pv = pu.limbs([e for x in pre for e in x]).reshape(count, arity, 4)
    pav = pu.limbs([e for x in paths for e in x]).reshape(count, depth, 4)
    rows = poseidon_merkle_leaf_assignments_host(curve.cid, pv, idx, pav, depth)
    s3 = 3 * au.SBOXES[arity]
    assert rows.shape == (count, poseidon_merkle_leaf_assignment_elems(arity, depth), 4) == (count, 2 + arity + s3 + 238 * depth, 4)
    assert pu.ints(rows[:, 1]) == [au.leaf_root(curve, pre[j], idx[j], paths[j]) for j in range(count)]
    assert np.array_equal(rows[:, 2:2 + arity], pv)
    for j in range(count):
        lv = 2 + arity + s3
        assert np.array_equal(rows[j, lv:lv + 238 * depth:238], pav[j])  # the siblings, at the level offsets the header states
        assert pu.ints(rows[j, lv + 1:lv + 1 + 238 * depth:238]) == [(idx[j] >> k) & 1 for k in range(depth)]
        assert np.array_equal(rows[j], witness_assignment(lambda: Circuit.merkle_leaf(curve.cid, depth, pre[j], idx[j], paths[j], witness_only=True))), j
    full = Circuit.merkle_leaf(curve.cid, depth, pre[1], idx[1], paths[1])
    try:
        assert np.array_equal(rows[1], full.arrays()["assignment"])
    finally:
        full.close()
    if depth == 1:
        assert np.array_equal(rows[2], ol.ints_to_limbs(au.poseidon_merkle_leaf_circuit(curve.fr, depth, pre[2], idx[2], paths[2]).assignment(), 4))


@CURVES
def test_argument_errors(curve):
    L = load_library()
    r = curve.fr.p
    p64 = ol.p64
    arity, depth = 3, 2
    x = pu.limbs(pu.random_elems(curve, arity, 1)).reshape(1, arity, 4)
    pa2 = pu.limbs(pu.random_elems(curve, depth, 2))
    idx = np.array([1], dtype=np.uint64)
    out = np.full((1, 2 + arity + 258 + 238 * depth, 4), 0xA5, dtype=np.uint64)
    fn = L.zl_poseidon_hash_assignments
    for a in (0, 1, 6):
        assert fn(None, curve.cid, a, p64(x), 1, p64(out)) == EINVAL
    assert fn(None, 77, arity, p64(x), 1, p64(out)) == EINVAL
    assert fn(None, curve.cid, arity, None, 1, p64(out)) == EINVAL
    assert fn(None, curve.cid, arity, p64(x), 1, None) == EINVAL
    assert (out == 0xA5).all()
    for pos in range(arity):
        for v in (r, (1 << 256) - 1):
            bad = x.copy()
            bad[0, pos] = pu.limbs([v])[0]
            assert fn(None, curve.cid, arity, p64(bad), 1, p64(out.copy())) == EINVAL
    assert fn(None, curve.cid, arity, None, 0, None) == 0
    assert fn(None, curve.cid, arity, p64(x), 0, p64(out)) == 0 and (out == 0xA5).all()
    assert fn(None, curve.cid, arity, p64(x), 1, p64(out)) == 0 and (out[0, 0] == [1, 0, 0, 0]).all()
    out[:] = 0xA5
    fn = L.zl_poseidon_merkle_leaf_assignments
    for a in (0, 1, 6):
        assert fn(None, curve.cid, a, p64(x), p64(idx), p64(pa2), depth, 1, p64(out)) == EINVAL
    for d in (0, 41):
        assert fn(None, curve.cid, arity, p64(x), p64(idx), p64(pu.limbs([1] * 41)), d, 1, p64(out)) == EINVAL
    assert fn(None, curve.cid, arity, p64(x), p64(np.array([4], dtype=np.uint64)), p64(pa2), depth, 1, p64(out)) == EINVAL  # index == 2^depth
    assert fn(None, 77, arity, p64(x), p64(idx), p64(pa2), depth, 1, p64(out)) == EINVAL
    for args in ((None, p64(idx), p64(pa2), p64(out)), (p64(x), None, p64(pa2), p64(out)), (p64(x), p64(idx), None, p64(out)), (p64(x), p64(idx), p64(pa2), None)):
        assert fn(None, curve.cid, arity, args[0], args[1], args[2], depth, 1, args[3]) == EINVAL
    assert (out == 0xA5).all()
    bad = x.copy()
    bad[0, 2] = pu.limbs([r])[0]
    assert fn(None, curve.cid, arity, p64(bad), p64(idx), p64(pa2), depth, 1, p64(out.copy())) == EINVAL
    bad_pa = pa2.copy()
    bad_pa[1] = pu.limbs([r])[0]
    assert fn(None, curve.cid, arity, p64(x), p64(idx), p64(bad_pa), depth, 1, p64(out.copy())) == EINVAL
    assert fn(None, curve.cid, arity, None, None, None, depth, 0, None) == 0
    assert fn(None, curve.cid, arity, p64(x), p64(idx), p64(pa2), depth, 1, p64(out)) == 0 and (out[0, 0] == [1, 0, 0, 0]).all()
    # the device-pointer forms never take the host path: a null ctx is refused
    assert L.zl_poseidon_hash_assignments_dev(None, curve.cid, arity, p64(x), 1, p64(out), out.shape[1]) == EINVAL
    assert L.zl_poseidon_merkle_leaf_assignments_dev(None, curve.cid, arity, p64(x), p64(idx), p64(pa2), depth, 1, p64(out), out.shape[1]) == EINVAL
    assert L.zl_poseidon_merkle_leaf_member_assignments_dev(None, curve.cid, arity, p64(pa2), p64(x), 1, depth, p64(idx), 1, p64(out), out.shape[1]) == EINVAL
