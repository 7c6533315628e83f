"""zl_groth16_prove_forest_members: memberships of leaves of a device Merkle forest in, proofs out.  Every proof must equal, byte for byte, what
zl_groth16_prove_merkle_members returns on that tree's node array at n = capacity for the same blinding scalars, on the device batch path (70 memberships, default
dispatch) and on the loop over the resident prover (5), and must verify against the root the call reports for it; keys of a chain or of another depth are
refused."""
import numpy as np
import pytest

import oracle_lib as ol
import poseidon_util as pu
from openzl_amd import BackendError, Circuit, Groth16Keys, MerkleForest

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
EINVAL = -1
TREES, DEPTH, CAPACITY = 5, 2, 4
LENS = [4, 3, 1, 2, 4]  # a full tree, absent siblings at both levels, a single leaf


def _same(p, q):
    return all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(p, q))


@pytest.fixture(scope="module")
def made(backend):
    """per curve, built once: depth-2 membership keys and a forest of five trees of lengths 4, 3, 1, 2, 4"""
    cache = {}

    def get(curve):
        if curve.cid not in cache:
            full = Circuit.merkle(curve.cid, DEPTH, 5, 1, [6, 7])
            keys = Groth16Keys(backend, full, seed=2991)
            forest = MerkleForest(backend, curve.cid, TREES, DEPTH, CAPACITY)
            tree_of = [t for t in range(TREES) for _ in range(LENS[t])]
            order = np.random.default_rng(5).permutation(len(tree_of))
            forest.append([tree_of[i] for i in order], pu.limbs(pu.random_elems(curve, len(tree_of), 7600)))
            assert [int(v) for v in forest.lens()] == LENS
            cache[curve.cid] = (full, keys, forest)
        return cache[curve.cid]

    yield get
    for full, keys, forest in cache.values():
        forest.close()
        keys.close()
        full.close()


def _items(count):
    tree_of = [(3 * j + 1) % TREES for j in range(count)]
    indices = [(j // TREES + j) % LENS[tree_of[j]] for j in range(count)]
    return tree_of, indices


@CURVES
@pytest.mark.parametrize("count", [70, 5], ids=["device-batch", "resident-loop"])
def test_proofs_equal_prove_merkle_members_per_tree_and_verify(backend, made, curve, count, monkeypatch):
    for k in ("ZL_TUNE_G16_BATCH_LOG_N", "ZL_TUNE_G16_BATCH_MIN", "ZL_TUNE_G16_BATCH_CHUNK", "ZL_TUNE_POSEIDON_CHUNK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("ZL_TUNE_POSEIDON_DEV_MIN", "0")
    full, keys, forest = made(curve)
    tree_of, indices = _items(count)
    assert set(tree_of) == set(range(TREES))
    rs = ol.random_scalars(curve, 2 * count, 7700 + count)
    r, s = np.ascontiguousarray(rs[:count]), np.ascontiguousarray(rs[count:])
    r[1], s[2] = 0, 0
    proofs, roots = keys.prove_forest_members(forest, tree_of, indices, r, s)
    assert len(proofs) == count and roots.shape == (count, 4)
    assert np.array_equal(roots, forest.roots()[tree_of])
    if count >= 64:
        with pytest.raises(BackendError) as e:
            backend.groth16_last_h(2)  # the device batch path ran: no single quotient
        assert e.value.code == EINVAL
    for t in range(TREES):
        sel = [j for j in range(count) if tree_of[j] == t]
        ref, root = keys.prove_merkle_members(forest.tree_nodes(t), CAPACITY, [indices[j] for j in sel], r[sel], s[sel])
        assert np.array_equal(root, forest.roots()[t])
        for j, p in zip(sel, ref):
            assert _same(proofs[j], p), (t, j)
    for j in range(count):
        assert keys.verify(proofs[j], roots[j]), j
    assert not keys.verify(proofs[0], roots[1 if tree_of[1] != tree_of[0] else 2])  # another tree's root is another statement
    lane = backend.fork()
    try:
        again, roots2 = keys.prove_forest_members(forest, tree_of, indices, r, s, lane=lane)
        assert all(_same(a, b) for a, b in zip(again, proofs)) and np.array_equal(roots2, roots)
    finally:
        lane.close()
        backend._forks.remove(lane)


@CURVES
def test_other_keys_and_bad_items_are_refused(backend, made, curve):
    full, keys, forest = made(curve)
    r = s = np.ascontiguousarray(ol.random_scalars(curve, 2, 7800))

    def refused(k, fr, tree_of, indices):
        if not getattr(k, "_r1cs", 0):
            k._r1cs = backend.r1cs_upload(curve.cid, k.circuit.arrays())
        with pytest.raises(BackendError) as e:
            backend._prove_forest_members(k.pk, curve.cid, k._r1cs, fr, tree_of, indices, r, s)
        assert e.value.code == EINVAL

    chain = Circuit(curve.cid, 1, 11, 2)
    chain_keys = Groth16Keys(backend, chain, seed=2992)
    shallow = Circuit.merkle(curve.cid, 1, 5, 1, [6])
    shallow_keys = Groth16Keys(backend, shallow, seed=2993)
    try:
        with pytest.raises(ValueError):
            chain_keys.prove_forest_members(forest, [0, 1], [0, 0], r, s)
        refused(chain_keys, forest, [0, 1], [0, 0])    # keys of a chain
        refused(shallow_keys, forest, [0, 1], [0, 0])  # keys of another depth
        refused(keys, forest, [0, 5], [0, 0])          # a tree id == trees
        refused(keys, forest, [0, 2], [0, 1])          # an index equal to that tree's length
        other = pu.CURVES[1] if curve is pu.CURVES[0] else pu.CURVES[0]
        with MerkleForest(backend, other.cid, TREES, DEPTH, CAPACITY) as wrong_curve, MerkleForest(None, curve.cid, TREES, DEPTH, CAPACITY) as mirror:
            wrong_curve.append([0, 1], pu.limbs([1, 2]))
            mirror.append([0, 1], pu.limbs([1, 2]))
            refused(keys, wrong_curve, [0, 1], [0, 0])
            refused(keys, mirror, [0, 1], [0, 0])      # a host-mirror forest
        proofs, roots = keys.prove_forest_members(forest, [], [], r[:0], s[:0])
        assert proofs == [] and roots.shape == (0, 4)
    finally:
        shallow_keys.close()
        shallow.close()
        chain_keys.close()
        chain.close()
