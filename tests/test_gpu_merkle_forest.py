"""The Merkle forest on the device (csrc/zl_poseidon_dev.hip: k_pos_forest_place / _level / _gather, ForestSrc) against its host mirror, which
tests/test_merkle_forest_host.py pins to the Python model: the shared append sequences through both append forms, the launch geometry of an append that
touches many trees (more segments than one wave, a range wider than one workgroup, one-leaf and untouched trees, several chunks), the existing _dev entry
points on one tree of the forest at n = capacity, rows across trees, the refusals -- which must leave the forest byte-identical -- and lanes / streams."""
import numpy as np
import pytest

import merkle_forest_util as fu
import poseidon_util as pu
from openzl_amd import BackendError, MerkleForest, poseidon_merkle_assignment_elems

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
EINVAL = -1
SENTINEL = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(autouse=True)
def device_path(monkeypatch):
    monkeypatch.setenv("ZL_TUNE_POSEIDON_DEV_MIN", "0")
    return monkeypatch


def dev(a: np.ndarray):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def host(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def _same_forest(a, b):
    assert [int(v) for v in a.lens()] == [int(v) for v in b.lens()]
    for t in range(a.trees):
        assert a.download(t).tobytes() == b.download(t).tobytes(), t
    assert a.roots().tobytes() == b.roots().tobytes()


@CURVES
@pytest.mark.parametrize("form", ["host-leaves", "device-leaves"])
@pytest.mark.parametrize("name", sorted(fu.SEQUENCES))
def test_sequences_equal_the_host_mirror(backend, curve, name, form):
    trees, depth, capacity, steps = fu.SEQUENCES[name]
    with MerkleForest(None, curve.cid, trees, depth, capacity) as mirror, MerkleForest(backend, curve.cid, trees, depth, capacity) as forest:
        _same_forest(forest, mirror)
        for tree_of, leaves in zip(steps, fu.sequence_leaves(curve, name)):
            lv = pu.limbs(leaves)
            mirror.append(tree_of, lv)
            if form == "host-leaves":
                forest.append(tree_of, lv)
            else:
                d_lv = dev(lv)
                forest.append_dev(tree_of, d_lv.data_ptr(), len(tree_of))
            _same_forest(forest, mirror)
        forest.append([], np.zeros((0, 4), dtype=np.uint64))
        forest.append_dev([], 0, 0)
        _same_forest(forest, mirror)


def _geometry_appends(curve):
    """(tree_of, leaves) of the two appends into 70 trees.  First: 200 leaves -- 130 to tree 0 (a level-1 range of 65 parents: more than one workgroup), ONE
    leaf each to the 64 trees 1 .. 64 (66 touched trees with tree 69: more segments than a wave has lanes), none to trees 65 .. 68, the last six to tree 69
    (the last tree); the trees are interleaved in the input.  Second, on top: 90 leaves -- 60 more to tree 0, a second leaf to trees 1 .. 20, a first one to
    tree 67, the rest to tree 69."""
    first = [0] * 130 + list(range(1, 65)) + [69] * 6
    second = [0] * 60 + list(range(1, 21)) + [67] + [69] * 9
    rng = np.random.default_rng(4242)
    out = []
    for k, tree_of in enumerate((first, second)):
        order = rng.permutation(len(tree_of))
        out.append(([tree_of[i] for i in order], pu.limbs(pu.random_elems(curve, len(tree_of), 7200 + k))))
    assert len(first) == 200 and len(second) == 90
    return out


@CURVES
@pytest.mark.parametrize("chunk", [None, "32"], ids=["chunk-default", "chunk-32"])
def test_launch_geometry_over_many_trees(backend, curve, chunk, device_path):
    if chunk is None:
        device_path.delenv("ZL_TUNE_POSEIDON_CHUNK", raising=False)
    else:
        device_path.setenv("ZL_TUNE_POSEIDON_CHUNK", chunk)  # seven staged chunks of leaves, three launches for tree 0's level 1 alone
    trees, depth, capacity = 70, 8, 256
    with MerkleForest(None, curve.cid, trees, depth, capacity) as mirror, MerkleForest(backend, curve.cid, trees, depth, capacity) as forest, \
            MerkleForest(backend, curve.cid, trees, depth, capacity) as forest_dev:
        for tree_of, lv in _geometry_appends(curve):
            mirror.append(tree_of, lv)
            forest.append(tree_of, lv)
            d_lv = dev(lv)
            forest_dev.append_dev(tree_of, d_lv.data_ptr(), len(tree_of))
            _same_forest(forest, mirror)
            _same_forest(forest_dev, mirror)
        lens = [int(v) for v in forest.lens()]
        assert lens[0] == 190 and lens[1:21] == [2] * 20 and lens[21:65] == [1] * 44 and lens[65:] == [0, 0, 1, 0, 15]
        for t in (65, 66, 68):  # an untouched tree stays all zero
            assert not forest.download(t).any() and not forest.roots()[t].any()


@CURVES
def test_existing_dev_calls_work_on_one_tree_at_n_equal_capacity(backend, curve):
    trees, depth, capacity = 3, 4, 11
    nv = poseidon_merkle_assignment_elems(depth)
    tree_of = [0] * 11 + [1] * 6 + [2]
    with MerkleForest(backend, curve.cid, trees, depth, capacity) as forest:
        forest.append(tree_of, pu.limbs(pu.random_elems(curve, len(tree_of), 7300)))
        items_t = [0] * 11 + [1] * 6 + [2]
        items_i = list(range(11)) + list(range(6)) + [0]
        own_paths = forest.paths(items_t, items_i)
        d_own = dev(np.full((len(items_t), nv, 4), SENTINEL, dtype=np.uint64))
        forest.member_assignments_dev(items_t, items_i, d_own.data_ptr())
        own_rows = host(d_own).reshape(len(items_t), nv, 4)
        at = 0
        for t, n in ((0, 11), (1, 6), (2, 1)):
            idx = list(range(n))
            assert np.array_equal(backend.poseidon_merkle_paths(curve.cid, forest.tree_nodes(t), capacity, depth, idx), own_paths[at:at + n])
            d_out = dev(np.full((n, nv, 4), SENTINEL, dtype=np.uint64))
            backend.poseidon_merkle_member_assignments_dev(curve.cid, forest.tree_nodes(t), capacity, depth, idx, d_out.data_ptr())
            rows = host(d_out).reshape(n, nv, 4)
            assert rows.tobytes() == own_rows[at:at + n].tobytes(), t   # rows across trees in one call == the per-tree calls, row by row
            assert np.array_equal(rows[:, 1], np.broadcast_to(forest.roots()[t], (n, 4)))  # [1] of every row is that tree's root
            at += n


@CURVES
def test_rows_across_trees_with_a_padded_stride_and_several_chunks(backend, curve, device_path):
    trees, depth, capacity = 5, 3, 6
    nv = poseidon_merkle_assignment_elems(depth)
    tree_of = [t for t in range(trees) for _ in range(t + 2)]  # lengths 2 .. 6
    with MerkleForest(backend, curve.cid, trees, depth, capacity) as forest:
        forest.append(tree_of, pu.limbs(pu.random_elems(curve, len(tree_of), 7400)))
        items_t = [(7 * j) % trees for j in range(70)]
        items_i = [(3 * j) % (items_t[j] + 2) for j in range(70)]
        d_ref = dev(np.zeros((70, nv, 4), dtype=np.uint64))
        forest.member_assignments_dev(items_t, items_i, d_ref.data_ptr())
        ref = host(d_ref).reshape(70, nv, 4)
        per_tree = {}
        for t in range(trees):
            d_out = dev(np.zeros((t + 2, nv, 4), dtype=np.uint64))
            backend.poseidon_merkle_member_assignments_dev(curve.cid, forest.tree_nodes(t), capacity, depth, list(range(t + 2)), d_out.data_ptr())
            per_tree[t] = host(d_out).reshape(t + 2, nv, 4)
        for j in range(70):
            assert ref[j].tobytes() == per_tree[items_t[j]][items_i[j]].tobytes(), j
        device_path.setenv("ZL_TUNE_POSEIDON_CHUNK", "32")
        stride = nv + 3
        d_out = dev(np.full((71, stride, 4), SENTINEL, dtype=np.uint64))
        forest.member_assignments_dev(items_t, items_i, d_out.data_ptr(), stride)
        out = host(d_out).reshape(71, stride, 4)
        assert out[:70, :nv].tobytes() == ref.tobytes()
        assert (out[:70, nv:] == SENTINEL).all() and (out[70] == SENTINEL).all()
        assert np.array_equal(forest.paths(items_t, items_i), np.stack([ref[j, 3 + 238 * np.arange(depth)] for j in range(70)]))  # a row's siblings are its path


@CURVES
def test_refusals_leave_the_forest_byte_identical(backend, curve, device_path):
    device_path.setenv("ZL_TUNE_POSEIDON_CHUNK", "32")
    trees, depth, capacity = 4, 7, 100
    vals = pu.random_elems(curve, 200, 7500)
    with MerkleForest(backend, curve.cid, trees, depth, capacity) as forest:
        forest.append([j % 3 for j in range(90)], pu.limbs(vals[:90]))  # 30 leaves in trees 0 .. 2
        snap = ([int(v) for v in forest.lens()], [forest.download(t).tobytes() for t in range(trees)])

        def refused(fn, *args):
            with pytest.raises(BackendError) as e:
                fn(*args)
            assert e.value.code == EINVAL
            assert ([int(v) for v in forest.lens()], [forest.download(t).tobytes() for t in range(trees)]) == snap

        bad = list(vals[90:190])  # 100 leaves = four chunks; the bad one lies in the third, behind 64 good ones
        bad[70] = curve.fr.p
        tree_of = [j % 4 for j in range(100)]
        d_bad = dev(pu.limbs(bad))
        refused(forest.append_dev, tree_of, d_bad.data_ptr(), 100)
        refused(forest.append, tree_of, pu.limbs(bad))
        d_good = dev(pu.limbs(vals[90:190]))
        refused(forest.append_dev, [0] * 71, d_good.data_ptr(), 71)       # tree 0 past its capacity by one leaf
        refused(forest.append_dev, [0, 4], d_good.data_ptr(), 2)          # a tree id == trees
        refused(forest.paths, [0, 3], [0, 0])                             # tree 3 is empty
        refused(forest.paths, [1], [30])                                  # an index equal to the length
        d_out = dev(np.zeros((1, poseidon_merkle_assignment_elems(depth), 4), dtype=np.uint64))
        refused(forest.member_assignments_dev, [1], [30], d_out.data_ptr())
        forest.append_dev(tree_of, d_good.data_ptr(), 100)               # the flag does not stick, and the same input without the bad leaf goes in
        with MerkleForest(None, curve.cid, trees, depth, capacity) as mirror:
            mirror.append([j % 3 for j in range(90)], pu.limbs(vals[:90]))
            mirror.append(tree_of, pu.limbs(vals[90:190]))
            _same_forest(forest, mirror)


@CURVES
def test_forked_lane_and_foreign_stream(backend, curve):
    import torch

    name = "three-trees-to-capacity"
    trees, depth, capacity, steps = fu.SEQUENCES[name]
    leaves = fu.sequence_leaves(curve, name)
    with MerkleForest(None, curve.cid, trees, depth, capacity) as mirror:
        for tree_of, lv in zip(steps, leaves):
            mirror.append(tree_of, pu.limbs(lv))
        lane = backend.fork()
        try:
            with MerkleForest(lane, curve.cid, trees, depth, capacity) as forest:
                for tree_of, lv in zip(steps, leaves):
                    forest.append(tree_of, pu.limbs(lv))
                _same_forest(forest, mirror)
                assert np.array_equal(forest.paths([2, 0], [7, 0]), mirror.paths([2, 0], [7, 0]))
        finally:
            lane.close()
            backend._forks.remove(lane)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            backend.set_stream(torch.cuda.current_stream().cuda_stream)
            try:
                with MerkleForest(backend, curve.cid, trees, depth, capacity) as forest:
                    for tree_of, lv in zip(steps, leaves):
                        d_lv = torch.from_numpy(pu.limbs(lv).view(np.int64).copy()).cuda(non_blocking=False)
                        forest.append_dev(tree_of, d_lv.data_ptr(), len(tree_of))
                    _same_forest(forest, mirror)
                    assert np.array_equal(forest.paths([2, 0], [7, 0]), mirror.paths([2, 0], [7, 0]))
            finally:
                backend.set_stream(0)
