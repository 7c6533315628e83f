"""Independent Python builder of the Merkle-membership circuit (zl_circuit_poseidon_merkle, include/zl_backend_ext.h) on top of the oracle's R1CS, LC and
Poseidon gadget, and the plain-Python fold for the expected root.  It pins the allocation order the header states -- level-major: sibling, Boolean index bit,
left = select(b, sib, cur), right = select(b, cur, sib), then the 234 S-box witnesses of H(left, right) -- and the rows of the two gadgets:
    Boolean  A = ONE - b, B = b,     C empty
    select   A = b,       B = t - f, C = out - f."""
import poseidon_util as pu
from oracle_lib import po


def _sub(a: po.LC, b: po.LC, p: int) -> po.LC:
    return a.add(b.scale(p - 1, p), p)


def new_boolean_witness(cs: po.R1CS, value: int) -> po.LC:
    """`value` is taken as it is (a test may pass 2): the row, not the allocation, is what keeps it Boolean"""
    p = cs.f.p
    b = cs.new_witness(value)
    cs.enforce(_sub(po.LC.const(1), b, p), b, po.LC())
    return b


def select(cs: po.R1CS, b: po.LC, t: po.LC, f: po.LC) -> po.LC:
    p = cs.f.p
    out = cs.new_witness(cs.value(t) if cs.value(b) else cs.value(f))
    cs.enforce(b, _sub(t, f, p), _sub(out, f, p))
    return out


def fold(curve, leaf: int, index: int, path) -> int:
    """the root: at level k the running digest joins on the right when bit k of index is set"""
    return pu.fold_path(curve, leaf, index, list(path))


def poseidon_merkle_circuit(field, depth: int, leaf: int, index: int, path, root=None, bits=None) -> po.R1CS:
    """root: the public input (default: the fold's value); bits: the values of the Boolean witnesses (default: the bits of index) -- both for negative tests"""
    assert len(path) == depth and 0 <= index < (1 << depth)
    curve = {c.fr.p: c for c in pu.CURVES}[field.p]
    keys, mds = pu.constants(curve.name)
    cs = po.R1CS(field)
    root_pub = cs.new_public(fold(curve, leaf, index, path) if root is None else root)
    cur = cs.new_witness(leaf)
    for j in range(depth):
        sib = cs.new_witness(path[j])
        b = new_boolean_witness(cs, (index >> j) & 1 if bits is None else bits[j])
        left = select(cs, b, sib, cur)
        right = select(cs, b, cur, sib)
        cur = po.poseidon_hash_gadget(cs, left, right, keys, mds)
    cs.enforce(cur, po.LC.const(1), root_pub)
    assert (cs.n_constraints, cs.n_instance, cs.n_witness) == (237 * depth + 1, 2, 1 + 238 * depth)
    return cs
