"""Independent Python builder of the two arity-general circuits (zl_circuit_poseidon_hash / zl_circuit_poseidon_merkle_leaf, include/zl_backend_ext.h) on top of
the oracle's R1CS and LC: a Poseidon gadget of any width of the specification table with the constants of tests/poseidon_arity_util.py, and the Boolean and
select rows of tests/merkle_circuit_util.py for the levels.  It pins what the header states:
    S-boxes are allocated in round order, lane order within a round, each as x^2, x^4, x^5; lane 0 of round 0 is a constant and folds;
    hash circuit:             public digest | the inputs, the 3 S(a) records | last row digest = public input
    leaf-membership circuit:  public root   | the preimage, the 3 S(a) records of the leaf hash (the leaf digest stays a linear combination), then per level
                              sibling, Boolean bit, left = select(b, sib, cur), right = select(b, cur, sib), the 234 records of H_2(left, right)."""
import merkle_circuit_util as mu
import poseidon_arity_util as pa
import poseidon_util as pu
from oracle_lib import po

# arity -> S(a): recorded S-boxes of one hash
SBOXES = {a: 8 * (a + 1) + pa.SPEC[a][2] - 1 for a in pa.ARITIES}
assert SBOXES == {2: 78, 3: 86, 4: 95, 5: 103}


def hash_shape(arity: int):
    """(n_constraints, n_instance, n_witness) of the hash circuit"""
    s3 = 3 * SBOXES[arity]
    return s3 + 1, 2, arity + s3


def leaf_shape(arity: int, depth: int):
    s3 = 3 * SBOXES[arity]
    return s3 + 237 * depth + 1, 2, arity + s3 + 238 * depth


def hash_gadget(cs: po.R1CS, curve, inputs) -> po.LC:
    """in-circuit hash of len(inputs) linear combinations: state (2^arity - 1, inputs), full MDS after every round, lane 0 out"""
    p = cs.f.p
    t = len(inputs) + 1
    keys, mds = pa.constants(curve.name, t)
    rf, rp = pa.rounds(t)
    state = [po.LC.const((1 << (t - 1)) - 1)] + list(inputs)
    half = rf // 2
    for rnd in range(rf + rp):
        state = [s.add(po.LC.const(keys[t * rnd + i]), p) for i, s in enumerate(state)]
        for i in (range(t) if rnd < half or rnd >= half + rp else range(1)):
            v = state[i]
            x2 = cs.mul(v, v)
            x4 = cs.mul(x2, x2)
            state[i] = cs.mul(x4, v)
        nxt = []
        for i in range(t):
            acc = po.LC()
            for j in range(t):
                acc = acc.add(state[j].scale(mds[i][j], p), p)
            nxt.append(acc)
        state = nxt
    return state[0]


def _curve_of(field):
    return {c.fr.p: c for c in pu.CURVES}[field.p]


def poseidon_hash_circuit(field, inputs, digest=None) -> po.R1CS:
    """digest: the public input (default: the hash's value) -- for negative tests"""
    curve = _curve_of(field)
    arity = len(inputs)
    cs = po.R1CS(field)
    pub = cs.new_public(pa.hash(curve, inputs) if digest is None else digest)
    xs = [cs.new_witness(v) for v in inputs]
    out = hash_gadget(cs, curve, xs)
    cs.enforce(out, po.LC.const(1), pub)
    assert (cs.n_constraints, cs.n_instance, cs.n_witness) == hash_shape(arity)
    return cs


def leaf_root(curve, preimage, index: int, path) -> int:
    return mu.fold(curve, pa.hash(curve, preimage), index, path)


def poseidon_merkle_leaf_circuit(field, depth: int, preimage, index: int, path, root=None) -> po.R1CS:
    assert len(path) == depth and 0 <= index < (1 << depth)
    curve = _curve_of(field)
    arity = len(preimage)
    keys2, mds2 = pu.constants(curve.name)
    cs = po.R1CS(field)
    root_pub = cs.new_public(leaf_root(curve, preimage, index, path) if root is None else root)
    xs = [cs.new_witness(v) for v in preimage]
    cur = hash_gadget(cs, curve, xs)
    for j in range(depth):
        sib = cs.new_witness(path[j])
        b = mu.new_boolean_witness(cs, (index >> j) & 1)
        left = mu.select(cs, b, sib, cur)
        right = mu.select(cs, b, cur, sib)
        cur = po.poseidon_hash_gadget(cs, left, right, keys2, mds2)
    cs.enforce(cur, po.LC.const(1), root_pub)
    assert (cs.n_constraints, cs.n_instance, cs.n_witness) == leaf_shape(arity, depth)
    return cs
