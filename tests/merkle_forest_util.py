"""Python model of the Merkle forest (include/zl_backend_ext.h: zl_merkle_forest_*) on top of poseidon_util.merkle_levels, and the append sequences the host
and the GPU tests share.  Per tree the expected node array has the layout of the forest's CAPACITY: level k holds ceil(capacity / 2^k) slots, the first
ceil(len / 2^k) of them are the model's nodes of a tree over the `len` leaves it has, every other slot is zero."""
import numpy as np

import poseidon_util as pu

_H = {}


def _hash2(curve, x, y):
    """pu.hash2, remembered: the sequences rebuild their trees after every append"""
    key = (curve.name, x, y)
    if key not in _H:
        _H[key] = pu.hash2(curve, x, y)
    return _H[key]


def tree_levels(curve, leaves, depth):
    return pu.merkle_levels(curve, leaves, depth, lambda x, y: _hash2(curve, x, y))


def expected_tree(curve, leaves, depth, capacity) -> np.ndarray:
    """(zl_poseidon_merkle_nodes(capacity, depth), 4) words: the node array of one tree of the forest holding `leaves`"""
    assert len(leaves) <= capacity <= 1 << depth
    levels = tree_levels(curve, leaves, depth)
    flat = []
    for k in range(depth + 1):
        size = -(-capacity // (1 << k))
        assert len(levels[k]) == -(-len(leaves) // (1 << k)) <= size
        flat += levels[k] + [0] * (size - len(levels[k]))
    assert len(flat) == pu.merkle_nodes(capacity, depth)
    return pu.limbs(flat)


class ForestModel:
    """the leaves of every tree, appended as zl_merkle_forest_append does: leaf i behind the leaves tree tree_of[i] already has, in input order"""

    def __init__(self, curve, trees, depth, capacity):
        self.curve, self.trees, self.depth, self.capacity = curve, trees, depth, capacity
        self.leaves = [[] for _ in range(trees)]

    def append(self, tree_of, leaves):
        for t, v in zip(tree_of, leaves):
            self.leaves[t].append(v)
        assert all(len(lv) <= self.capacity for lv in self.leaves)

    def lens(self):
        return [len(lv) for lv in self.leaves]

    def tree(self, t) -> np.ndarray:
        return expected_tree(self.curve, self.leaves[t], self.depth, self.capacity)

    def root(self, t) -> int:
        return pu.merkle_root(tree_levels(self.curve, self.leaves[t], self.depth))


# name -> (trees, depth, capacity, steps); a step is the tree_of of one append
SEQUENCES = {
    # per-tree lengths 0 -> 1 -> 2 -> 3 -> 5 -> 8: a single leaf into an empty tree, odd / even boundaries, fill to capacity; the trees interleaved
    "three-trees-to-capacity": (3, 3, 8, [[0, 1, 2], [2, 0, 1], [1, 2, 0], [0, 1, 2, 2, 1, 0], [0, 0, 0, 1, 2, 1, 2, 1, 2]]),
    # capacity 5 at depth 5: levels of 5, 3, 2, 1, 1, 1 slots -- leaf 4 and node (1, 2) have a right sibling beyond their level
    "right-child-beyond-the-level": (2, 5, 5, [[0, 0, 1], [0, 1, 1], [0, 0, 1, 1]]),
    # capacity 3 at depth 6: four levels above a single node
    "levels-above-a-single-node": (2, 6, 3, [[0], [0, 1], [0, 1, 1]]),
    # the second and third appends leave trees 0 and 2 (then 0, 1, 3) alone
    "some-trees-untouched": (4, 3, 8, [[0, 1, 2, 3, 0, 1], [1, 1, 3], [2]]),
}


def sequence_leaves(curve, name):
    """the leaves of every step of a sequence, from one seeded pool; 0 and r - 1 among the first"""
    trees, depth, capacity, steps = SEQUENCES[name]
    pool = pu.random_elems(curve, sum(len(s) for s in steps), 7000 + sorted(SEQUENCES).index(name))
    pool[0], pool[1] = 0, curve.fr.p - 1
    out, at = [], 0
    for s in steps:
        out.append(pool[at:at + len(s)])
        at += len(s)
    return out


def all_trees(forest) -> list:
    return [forest.download(t) for t in range(forest.trees)]
