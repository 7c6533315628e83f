"""Batched Poseidon through its host path (ctx == NULL: the host mirror's permutation over the library's thread pool, no device): layouts, the Merkle
rules and every argument check of include/zl_backend_ext.h, against the Python model of tests/poseidon_util.py -- which is itself pinned here to
po.poseidon_permute, the reference's own [3, 1, 2] vector and a hand-unrolled depth-3 tree."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle_lib as ol
import poseidon_util as pu
from oracle_lib import po
from openzl_amd import Circuit
from openzl_amd import backend as zb

HERE = os.path.dirname(os.path.abspath(__file__))
FX = json.load(open(os.path.join(HERE, "golden", "ref_poseidon_fixtures.json")))
CURVES = pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
EINVAL = -1


def edge_and_random(curve, n, seed):
    """n elements: 0, 1, r - 1 first, then seeded random ones"""
    return ([0, 1, curve.fr.p - 1] + pu.random_elems(curve, n, seed))[:n]


# ---- the helper is pinned first ---------------------------------------------------------------------------------------------------------------------
@CURVES
def test_helper_equals_the_oracle_permutation(curve):
    for st in ([3, 1, 2], [curve.fr.p - 1, 0, 0x1234567890ABCDEF << 100]):
        assert pu.permute(curve, st) == po.poseidon_permute(curve.fr, st)


def test_helper_equals_the_reference_vector():
    fx = FX["permutation_width3"]
    assert [int(v) for v in fx["input"]] == [3, 1, 2]
    assert [str(v) for v in pu.permute(po.BLS12_381, [3, 1, 2])] == fx["output"]
    assert str(pu.hash2(po.BLS12_381, 1, 2)) == fx["output"][0]


@CURVES
def test_helper_merkle_root_equals_hand_unrolled_depth_3(curve):
    H = lambda x, y: pu.hash2(curve, x, y)  # noqa: E731
    a, b, c, d, e = pu.random_elems(curve, 5, 11)
    lv = pu.merkle_levels(curve, [a, b, c, d, e], 3)
    # five leaves: the third node of level 1 has no right child, the second node of level 2 no right child either (its sibling subtree holds no leaf)
    assert pu.merkle_root(lv) == H(H(H(a, b), H(c, d)), H(H(e, 0), 0))
    assert [len(x) for x in lv] == [5, 3, 2, 1] and pu.merkle_nodes(5, 3) == 11
    assert pu.merkle_path(lv, 4) == [0, 0, H(H(a, b), H(c, d))]
    assert pu.merkle_path(lv, 2) == [d, H(a, b), H(H(e, 0), 0)]
    assert pu.fold_path(curve, e, 4, pu.merkle_path(lv, 4)) == pu.merkle_root(lv)


# ---- permute / hash2 / chain ------------------------------------------------------------------------------------------------------------------------
@CURVES
@pytest.mark.parametrize("count", [0, 1, 3, 100])
def test_permute_hash2_chain_host(curve, count):
    vals = edge_and_random(curve, 3 * count, 21)
    states = [vals[3 * i:3 * i + 3] for i in range(count)]
    got = zb.poseidon_permute_batch_host(curve.cid, pu.limbs(vals))
    assert got.shape == (count, 3, 4)
    assert [pu.ints(g) for g in got] == [pu.permute(curve, s) for s in states]
    pairs = [(vals[2 * i], vals[2 * i + 1]) for i in range(count)]
    got = zb.poseidon_hash2_host(curve.cid, pu.limbs(vals[:2 * count]))
    assert pu.ints(got) == [pu.hash2(curve, x, y) for x, y in pairs]
    for k in (1, 3):
        got = zb.poseidon_chain_host(curve.cid, pu.limbs([p[0] for p in pairs]), pu.limbs([p[1] for p in pairs]), k)
        assert pu.ints(got) == [pu.chain(curve, x, y, k) for x, y in pairs]


def test_hash2_of_1_2_is_the_reference_digest():
    assert str(pu.ints(zb.poseidon_hash2_host(po.BLS12_381.cid, pu.limbs([1, 2])))[0]) == FX["permutation_width3"]["output"][0]


@CURVES
def test_canonical_edges_pass_and_values_from_r_on_are_refused(curve):
    r = curve.fr.p
    for pos in range(3):
        for v, ok in ((0, True), (1, True), (r - 1, True), (r, False), ((1 << 256) - 1, False)):
            st = [5, 6, 7]
            st[pos] = v
            if ok:
                assert pu.ints(zb.poseidon_permute_batch_host(curve.cid, pu.limbs(st))[0]) == pu.permute(curve, st)
            else:
                with pytest.raises(zb.BackendError) as e:
                    zb.poseidon_permute_batch_host(curve.cid, pu.limbs(st))
                assert e.value.code == EINVAL
    for bad in (r, (1 << 256) - 1):
        for call in (lambda: zb.poseidon_hash2_host(curve.cid, pu.limbs([1, 2, 3, bad])), lambda: zb.poseidon_hash2_host(curve.cid, pu.limbs([bad, 2])),
                     lambda: zb.poseidon_chain_host(curve.cid, pu.limbs([bad]), pu.limbs([1]), 2), lambda: zb.poseidon_chain_host(curve.cid, pu.limbs([1]), pu.limbs([bad]), 2),
                     lambda: zb.poseidon_merkle_root_host(curve.cid, pu.limbs([1, bad, 3]), 2),
                     lambda: zb.poseidon_roots_from_paths_host(curve.cid, pu.limbs([bad]), [0], pu.limbs([1, 2]), 2),
                     lambda: zb.poseidon_roots_from_paths_host(curve.cid, pu.limbs([1]), [0], pu.limbs([1, bad]), 2)):
            with pytest.raises(zb.BackendError) as e:
                call()
            assert e.value.code == EINVAL


@CURVES
@pytest.mark.parametrize("k", [1, 2, 8])
def test_chain_is_the_public_input_of_the_chain_circuit(curve, k):
    x0, x1 = pu.random_elems(curve, 2, 31 + k)
    c = Circuit(curve.cid, k, x0, x1)
    try:
        a = c.arrays()
        assert a["n_instance"] == 2
        pub = ol.limbs_to_ints(np.asarray(a["assignment"]).reshape(-1, 4)[1:2])[0]
    finally:
        c.close()
    assert pu.ints(zb.poseidon_chain_host(curve.cid, pu.limbs([x0]), pu.limbs([x1]), k)) == [pub] == [pu.chain(curve, x0, x1, k)]


# ---- Merkle -----------------------------------------------------------------------------------------------------------------------------------------
def test_merkle_nodes_formula():
    for depth in (1, 3, 10):
        for n in (0, 1, 2, 3, 5, 1000):
            exp = pu.merkle_nodes(n, depth) if n <= (1 << depth) else 0
            assert zb.poseidon_merkle_nodes(n, depth) == exp, (n, depth)
    assert zb.poseidon_merkle_nodes(4, 0) == 0 and zb.poseidon_merkle_nodes(4, 41) == 0 and zb.poseidon_merkle_nodes(1, 40) == 41
    assert zb.poseidon_merkle_nodes(1 << 10, 10) == 2047


@CURVES
def test_merkle_roots_paths_and_folds_at_depth_4(curve):
    depth = 4
    leaves = pu.random_elems(curve, 16, 41)
    for n in range(0, 17):
        lv = pu.merkle_levels(curve, leaves[:n], depth)
        nodes, root = zb.poseidon_merkle_build_host(curve.cid, pu.limbs(leaves[:n]), depth)
        assert pu.ints(nodes) == pu.merkle_flat(lv), n
        assert pu.ints(root) == [pu.merkle_root(lv)] == pu.ints(zb.poseidon_merkle_root_host(curve.cid, pu.limbs(leaves[:n]), depth)), n
        if n == 0:
            assert zb.poseidon_merkle_paths_host(nodes, 0, depth, []).shape == (0, depth, 4)
            continue
        idx = list(range(n))
        paths = zb.poseidon_merkle_paths_host(nodes, n, depth, idx)
        assert [pu.ints(p) for p in paths] == [pu.merkle_path(lv, i) for i in idx], n
        roots = zb.poseidon_roots_from_paths_host(curve.cid, pu.limbs(leaves[:n]), idx, paths, depth)
        assert pu.ints(roots) == [pu.merkle_root(lv)] * n, n
        # a flipped sibling, a wrong index bit
        bad = paths.copy()
        bad[n - 1, depth - 1, 0] ^= np.uint64(1)
        assert pu.ints(zb.poseidon_roots_from_paths_host(curve.cid, pu.limbs(leaves[:n]), idx, bad, depth))[n - 1] != pu.merkle_root(lv)
        assert pu.ints(roots[: n - 1]) == pu.ints(zb.poseidon_roots_from_paths_host(curve.cid, pu.limbs(leaves[:n]), idx, bad, depth)[: n - 1])
        flipped = [i ^ 2 for i in idx]
        got = pu.ints(zb.poseidon_roots_from_paths_host(curve.cid, pu.limbs(leaves[:n]), flipped, paths, depth))
        assert all(g != pu.merkle_root(lv) for g in got), n


@CURVES
def test_depth_beyond_the_leaves_is_a_run_of_right_zero_joins(curve):
    leaves = pu.random_elems(curve, 3, 43)
    H = lambda x, y: pu.hash2(curve, x, y)  # noqa: E731
    exp = H(H(leaves[0], leaves[1]), H(leaves[2], 0))
    for _ in range(4):
        exp = H(exp, 0)
    assert pu.ints(zb.poseidon_merkle_root_host(curve.cid, pu.limbs(leaves), 6)) == [exp]


# ---- arguments --------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    L = zb.load_library()
    one = np.zeros((4, 4), dtype=np.uint64)
    out = np.zeros((64, 4), dtype=np.uint64)
    idx = np.zeros(4, dtype=np.uint64)
    p, o, ix = ol.p64(one), ol.p64(out), ol.p64(idx)
    # count == 0: ZL_OK even with null pointers, nothing written
    assert L.zl_poseidon_permute_batch(None, 1, None, 0) == 0
    assert L.zl_poseidon_hash2_batch(None, 1, None, 0, None) == 0
    assert L.zl_poseidon_chain_batch(None, 2, None, None, 1, 0, None) == 0
    assert L.zl_poseidon_merkle_roots_from_paths(None, 1, None, None, None, 3, 0, None) == 0
    assert L.zl_poseidon_merkle_paths(None, 4, 2, None, 0, None) == 0
    assert not out.any()
    # unknown curve
    for curve in (0, 3, 99):
        assert L.zl_poseidon_permute_batch(None, curve, p, 1) == EINVAL
        assert L.zl_poseidon_hash2_batch(None, curve, p, 1, o) == EINVAL
        assert L.zl_poseidon_chain_batch(None, curve, p, p, 1, 1, o) == EINVAL
        assert L.zl_poseidon_merkle_root(None, curve, p, 2, 2, o) == EINVAL
        assert L.zl_poseidon_merkle_build(None, curve, p, 2, 2, o, o) == EINVAL
        assert L.zl_poseidon_merkle_roots_from_paths(None, curve, p, ix, p, 2, 1, o) == EINVAL
    # null pointers
    assert L.zl_poseidon_permute_batch(None, 1, None, 1) == EINVAL
    assert L.zl_poseidon_hash2_batch(None, 1, None, 1, o) == EINVAL and L.zl_poseidon_hash2_batch(None, 1, p, 1, None) == EINVAL
    assert L.zl_poseidon_chain_batch(None, 1, None, p, 1, 1, o) == EINVAL and L.zl_poseidon_chain_batch(None, 1, p, None, 1, 1, o) == EINVAL
    assert L.zl_poseidon_chain_batch(None, 1, p, p, 1, 1, None) == EINVAL
    assert L.zl_poseidon_merkle_root(None, 1, None, 2, 2, o) == EINVAL and L.zl_poseidon_merkle_root(None, 1, p, 2, 2, None) == EINVAL
    assert L.zl_poseidon_merkle_build(None, 1, p, 2, 2, None, o) == EINVAL and L.zl_poseidon_merkle_build(None, 1, p, 2, 2, o, None) == EINVAL
    assert L.zl_poseidon_merkle_roots_from_paths(None, 1, None, ix, p, 2, 1, o) == EINVAL
    assert L.zl_poseidon_merkle_roots_from_paths(None, 1, p, None, p, 2, 1, o) == EINVAL
    assert L.zl_poseidon_merkle_roots_from_paths(None, 1, p, ix, None, 2, 1, o) == EINVAL
    assert L.zl_poseidon_merkle_roots_from_paths(None, 1, p, ix, p, 2, 1, None) == EINVAL
    assert L.zl_poseidon_merkle_paths(None, 4, 2, ix, 1, o) == EINVAL and L.zl_poseidon_merkle_paths(p, 4, 2, None, 1, o) == EINVAL
    assert L.zl_poseidon_merkle_paths(p, 4, 2, ix, 1, None) == EINVAL
    # chain of no links: as zl_circuit_poseidon_chain
    assert L.zl_poseidon_chain_batch(None, 1, p, p, 0, 1, o) == EINVAL
    # depth outside 1..40, n > 2^depth
    for depth in (0, 41):
        assert L.zl_poseidon_merkle_root(None, 1, p, 1, depth, o) == EINVAL
        assert L.zl_poseidon_merkle_build(None, 1, p, 1, depth, o, o) == EINVAL
        assert L.zl_poseidon_merkle_roots_from_paths(None, 1, p, ix, p, depth, 1, o) == EINVAL
        assert L.zl_poseidon_merkle_paths(p, 1, depth, ix, 1, o) == EINVAL
    assert L.zl_poseidon_merkle_root(None, 1, p, 3, 1, o) == EINVAL and L.zl_poseidon_merkle_build(None, 1, p, 3, 1, o, o) == EINVAL
    assert L.zl_poseidon_merkle_root(None, 1, p, 2, 1, o) == 0
    # a leaf index at or above n (paths), at or above 2^depth (fold): before any work
    nodes = np.zeros((7, 4), dtype=np.uint64)
    idx[:] = [0, 1, 3, 0]
    fresh = np.zeros((8, 4), dtype=np.uint64)
    assert L.zl_poseidon_merkle_paths(ol.p64(nodes), 3, 2, ix, 3, ol.p64(fresh)) == EINVAL and not fresh.any()
    assert L.zl_poseidon_merkle_paths(ol.p64(nodes), 3, 2, ix, 2, ol.p64(fresh)) == 0
    idx[:] = [0, 4, 0, 0]
    assert L.zl_poseidon_merkle_roots_from_paths(None, 1, p, ix, o, 2, 2, o) == EINVAL
    # n == 0: the zero digest
    root = np.ones(4, dtype=np.uint64)
    assert L.zl_poseidon_merkle_root(None, 1, None, 0, 5, ol.p64(root)) == 0 and not root.any()
    # the device-pointer forms have no host path
    assert L.zl_poseidon_hash2_batch_dev(None, 1, C.c_void_p(8), 1, C.c_void_p(8)) == EINVAL
    assert L.zl_poseidon_merkle_build_dev(None, 1, C.c_void_p(8), 1, 1, C.c_void_p(8), o) == EINVAL
    assert L.zl_poseidon_merkle_paths_dev(None, 1, C.c_void_p(8), 1, 1, ix, 1, o) == EINVAL
