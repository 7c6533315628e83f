"""Python model of the batched Poseidon entry points (include/zl_backend_ext.h): the width-3 permutation with the LFSR constants generated ONCE per field
(po.poseidon_permute regenerates them on every call), the arity-2 hash H(x, y) = permute([3, x, y])[0], the hash chain, and the Merkle tree / path / fold
rules exactly as the header states them.  Plain Python integers; pinned by tests/test_poseidon_host.py against po.poseidon_permute, the reference's own
[3, 1, 2] vector and a hand-unrolled depth-3 tree."""
import functools

import numpy as np

import oracle_lib as ol
from oracle_lib import po

RF, RP = 8, 55
CURVES = [po.BLS12_381, po.BN254]


@functools.lru_cache(maxsize=None)
def constants(curve_name: str):
    curve = {c.name: c for c in CURVES}[curve_name]
    return po.poseidon_round_constants(curve.fr, 3, RF, RP), po.poseidon_mds(curve.fr, 3)


def permute(curve, state):
    keys, mds = constants(curve.name)
    p = curve.fr.p
    s0, s1, s2 = (v % p for v in state)
    half = RF // 2
    for rnd in range(RF + RP):
        s0, s1, s2 = (s0 + keys[3 * rnd]) % p, (s1 + keys[3 * rnd + 1]) % p, (s2 + keys[3 * rnd + 2]) % p
        s0 = pow(s0, 5, p)
        if rnd < half or rnd >= half + RP:
            s1, s2 = pow(s1, 5, p), pow(s2, 5, p)
        s0, s1, s2 = ((m[0] * s0 + m[1] * s1 + m[2] * s2) % p for m in mds)
    return [s0, s1, s2]


def hash2(curve, x, y):
    return permute(curve, [3, x, y])[0]


def chain(curve, x0, x1, k):
    h = x0
    for _ in range(k):
        h = hash2(curve, h, x1)
    return h


def merkle_nodes(n, depth):
    """the element count of the node array: levels 0 .. depth of ceil(n / 2^k) nodes"""
    return sum(-(-n // (1 << k)) for k in range(depth + 1))


def merkle_levels(curve, leaves, depth, hash_fn=None):
    """levels[k][j]: level 0 = the leaves, node(k, j) = H(node(k-1, 2j), node(k-1, 2j+1) or 0); absent nodes are simply not in the lists"""
    h = hash_fn or (lambda x, y: hash2(curve, x, y))
    levels = [list(leaves)]
    for _ in range(depth):
        c = levels[-1]
        levels.append([h(c[2 * j], c[2 * j + 1] if 2 * j + 1 < len(c) else 0) for j in range((len(c) + 1) // 2)])
    return levels


def merkle_root(levels):
    return levels[-1][0] if levels[-1] else 0


def merkle_flat(levels):
    return [v for lv in levels for v in lv]


def merkle_path(levels, index):
    """the siblings of leaf `index` from the bottom up (depth entries), zero where the tree has no such node"""
    out = []
    for k in range(len(levels) - 1):
        sib = (index >> k) ^ 1
        out.append(levels[k][sib] if sib < len(levels[k]) else 0)
    return out


def fold_path(curve, leaf, index, path, hash_fn=None):
    h = hash_fn or (lambda x, y: hash2(curve, x, y))
    cur = leaf
    for k, sib in enumerate(path):
        cur = h(sib, cur) if (index >> k) & 1 else h(cur, sib)
    return cur


# ---- limbs -------------------------------------------------------------------------------------------------------------------------------------
def limbs(vals) -> np.ndarray:
    """ints -> (len, 4) uint64 canonical words (works for any value below 2^256, canonical or not)"""
    vals = list(vals)
    return ol.ints_to_limbs(vals, 4) if vals else np.zeros((0, 4), dtype=np.uint64)


def ints(a) -> list:
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
    return ol.limbs_to_ints(a) if a.shape[0] else []


def random_elems(curve, n, seed):
    """n field elements below r from a seeded generator"""
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "little") % curve.fr.p for _ in range(n)]


def host_hash2_loop(curve, pairs):
    """H over pairs through the EXISTING one-at-a-time host entry point zl_poseidon_permute (tests/test_host_mirror.py pins it to the oracle): the expectation
    for cases with more hashes than the Python model should compute"""
    from openzl_amd import poseidon_permute

    out = []
    for x, y in pairs:
        out.append(ol.limbs_to_ints(poseidon_permute(curve.cid, ol.ints_to_limbs([3, x, y], 4)))[0])
    return out


def host_loop_hash_fn(curve):
    return lambda x, y: host_hash2_loop(curve, [(x, y)])[0]
