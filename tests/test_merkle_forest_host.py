"""The host mirror of the Merkle forest (zl_merkle_forest_* with a NULL ctx) against the Python model of tests/merkle_forest_util.py: the full node array of
every tree after every append, the equivalence with the existing Merkle family (roots, paths, folds), and the refusals, which must leave lengths and nodes as
they were.  No device."""
import ctypes as C

import numpy as np
import pytest

import merkle_forest_util as fu
import poseidon_util as pu
from openzl_amd import (BackendError, MerkleForest, load_library, poseidon_merkle_build_host, poseidon_merkle_nodes, poseidon_merkle_paths_host,
                        poseidon_merkle_root_host, poseidon_roots_from_paths_host)

CURVES = pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
EINVAL = -1


def _snapshot(forest):
    return [int(v) for v in forest.lens()], [t.tobytes() for t in fu.all_trees(forest)]


@CURVES
@pytest.mark.parametrize("name", sorted(fu.SEQUENCES))
def test_full_node_arrays_after_every_append(curve, name):
    trees, depth, capacity, steps = fu.SEQUENCES[name]
    model = fu.ForestModel(curve, trees, depth, capacity)
    with MerkleForest(None, curve.cid, trees, depth, capacity) as forest:
        assert (forest.trees, forest.depth, forest.capacity, forest.tree_stride) == (trees, depth, capacity, poseidon_merkle_nodes(capacity, depth))
        assert not any(t.any() for t in fu.all_trees(forest)) and not forest.roots().any()  # empty trees: all zero, the roots too
        for tree_of, leaves in zip(steps, fu.sequence_leaves(curve, name)):
            before = fu.all_trees(forest)
            forest.append(tree_of, pu.limbs(leaves))
            model.append(tree_of, leaves)
            assert [int(v) for v in forest.lens()] == model.lens()
            for t in range(trees):
                got = forest.download(t)
                assert got.tobytes() == model.tree(t).tobytes(), (name, tree_of, t)
                if t not in tree_of:
                    assert got.tobytes() == before[t].tobytes(), (name, tree_of, t)
            assert pu.ints(forest.roots()) == [model.root(t) for t in range(trees)]
    if name == "three-trees-to-capacity":
        assert model.lens() == [capacity] * trees


@CURVES
def test_roots_and_paths_are_those_of_the_merkle_family(curve):
    name = "right-child-beyond-the-level"
    trees, depth, capacity, steps = fu.SEQUENCES[name]
    model = fu.ForestModel(curve, trees, depth, capacity)
    with MerkleForest(None, curve.cid, trees, depth, capacity) as forest:
        for tree_of, leaves in zip(steps[:2], fu.sequence_leaves(curve, name)):  # lengths 3 and 3 of 5: absent siblings inside the capacity's levels
            forest.append(tree_of, pu.limbs(leaves))
            model.append(tree_of, leaves)
        roots = forest.roots()
        tree_of = [t for t in range(trees) for _ in model.leaves[t]]
        indices = [i for t in range(trees) for i in range(len(model.leaves[t]))]
        paths = forest.paths(tree_of, indices)
        assert paths.shape == (len(indices), depth, 4)
        at = 0
        for t in range(trees):
            lv = pu.limbs(model.leaves[t])
            n = len(model.leaves[t])
            assert np.array_equal(roots[t], poseidon_merkle_root_host(curve.cid, lv, depth))
            nodes, root = poseidon_merkle_build_host(curve.cid, lv, depth)  # a fresh build: the layout of n = len
            assert np.array_equal(root, roots[t])
            assert np.array_equal(paths[at:at + n], poseidon_merkle_paths_host(nodes, n, depth, list(range(n))))
            # ... and the gather over the forest's own array at n = capacity is the same gather
            assert np.array_equal(paths[at:at + n], poseidon_merkle_paths_host(forest.download(t), capacity, depth, list(range(n))))
            at += n
        leaves = pu.limbs([v for t in range(trees) for v in model.leaves[t]])
        folded = poseidon_roots_from_paths_host(curve.cid, leaves, indices, paths, depth)
        assert np.array_equal(folded, roots[tree_of])
        assert forest.paths([], []).shape == (0, depth, 4)


@CURVES
def test_refusals_leave_lengths_and_nodes_as_they_were(curve):
    trees, depth, capacity = 3, 3, 8
    r = curve.fr.p
    vals = pu.random_elems(curve, 12, 7100)
    with MerkleForest(None, curve.cid, trees, depth, capacity) as forest:
        forest.append([0, 0, 0, 1, 0, 0, 0, 0], pu.limbs(vals[:8]))  # tree 0 holds 7, tree 1 one leaf
        snap = _snapshot(forest)
        assert snap[0] == [7, 1, 0]

        def refused(fn, *args):
            with pytest.raises(BackendError) as e:
                fn(*args)
            assert e.value.code == EINVAL
            assert _snapshot(forest) == snap

        refused(forest.append, [1, 3], pu.limbs(vals[8:10]))            # a tree id == trees, behind a good one
        refused(forest.append, [2, 0, 0], pu.limbs(vals[8:11]))         # tree 0 past its capacity by one leaf
        refused(forest.append, [1, 2, 1], pu.limbs([vals[8], r, vals[9]]))  # a leaf equal to r in the middle
        refused(forest.append, [1], pu.limbs([(1 << 256) - 1]))
        refused(forest.paths, [0, 1], [6, 1])                           # an index equal to that tree's length
        refused(forest.paths, [0, 2], [0, 0])                           # ... an empty tree has no leaf 0
        refused(forest.paths, [3], [0])
        refused(forest.append_dev, [1], 4096, 1)                        # device leaves into a host-mirror forest
        refused(forest.member_assignments_dev, [0], [0], 4096)          # rows are written by the device only
        forest.append([0], pu.limbs(vals[11:12]))                      # the forest still works: tree 0 is now full
        assert [int(v) for v in forest.lens()] == [8, 1, 0]
        assert forest.download(0).tobytes() == fu.expected_tree(curve, vals[:3] + vals[4:8] + vals[11:12], depth, capacity).tobytes()


def test_trivial_cases_and_bad_shapes():
    L = load_library()
    assert L.zl_merkle_forest_destroy(None) is None
    curve = pu.CURVES[0]
    with MerkleForest(None, curve.cid, 2, 4, 9) as forest:
        forest.append([], np.zeros((0, 4), dtype=np.uint64))  # count == 0
        assert L.zl_merkle_forest_append(forest._f, None, None, 0) == 0
        assert [int(v) for v in forest.lens()] == [0, 0] and not forest.roots().any()
        assert forest.tree_nodes(1) - forest.tree_nodes(0) == forest.tree_stride * 32
        with pytest.raises(BackendError):
            forest.tree_nodes(2)
        with pytest.raises(BackendError):
            forest.download(2)
    out = C.c_void_p()
    for curve_id, trees, depth, capacity in ((9, 1, 3, 8), (1, 0, 3, 8), (1, 65537, 3, 8), (1, 1, 0, 1), (1, 1, 41, 8), (1, 1, 3, 0), (1, 1, 3, 9)):
        assert L.zl_merkle_forest_create(None, curve_id, trees, depth, capacity, C.byref(out)) == EINVAL and not out.value
    assert L.zl_merkle_forest_create(None, 1, 65536, 40, 1 << 40, C.byref(out)) == -2 and not out.value  # ZL_ENOMEM: 2^62 bytes of nodes
    assert L.zl_merkle_forest_create(None, 1, 1, 3, 8, None) == EINVAL
    assert L.zl_merkle_forest_describe(None, None, None, None, None) == EINVAL
    assert L.zl_merkle_forest_lens(None, None) == EINVAL and L.zl_merkle_forest_roots(None, None) == EINVAL
    assert L.zl_groth16_prove_forest_members(None, None, 0, None, None, None, None, None, 0, None, None) == EINVAL
