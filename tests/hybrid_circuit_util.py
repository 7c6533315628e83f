"""Independent Python builder of the hybrid-encryption circuit (zl_circuit_hybrid_encrypt, include/zl_backend_ext.h) on the oracle's R1CS and LC.  It takes
the point gadgets of tests/ed_circuit_util.py (double, add), the Boolean and select rows of tests/merkle_circuit_util.py, the permutation gadget of
tests/poseidon_duplex_util.py and the model of tests/edwards_util.py (hybrid_encrypt) and COMPOSES the rows itself, in the order the header states:
    publics    G.x G.y  pk.x pk.y  epk.x epk.y  tag  ciphertext  header
    witnesses  esk, its bits (once), the ladder over G, the ladder over pk (its last R is the key S), the plaintext, the cipher's S-box records
    rows       the bits', sum 2^i b_i = esk, the G ladder's, epk bound, the pk ladder's, the cipher's records, tag = public tag, one per ciphertext element"""
import edwards_util as eu
import ed_circuit_util as ec
import merkle_circuit_util as mu
import poseidon_duplex_util as du
import poseidon_util as pu
from oracle_lib import po


def sbox_records(width: int, header_len: int, blocks: int) -> int:
    """S of the header: (F - 1 - Z) + (SB + N - 1) F at K = 2, Z = max(0, rate - 2)"""
    f = du.sboxes(width)
    return (f - 1 - max(0, width - 1 - 2)) + (du.permutations(width, 2, header_len, blocks) - 1) * f


def shape(width: int, bits: int, header_len: int, blocks: int):
    """(n_constraints, n_instance, n_witness), counted from the header's lists of rows and witnesses -- NOT from its closed formulas:
    rows      bits + 1 + L + 2 + L + 3 S + 1 + T      with L = 2 + 13 (bits - 1) per ladder and T = N rate
    witnesses 1 + bits + 2 L + T + 3 S"""
    t, s, lad = blocks * (width - 1), sbox_records(width, header_len, blocks), 2 + 13 * (bits - 1)
    return bits + 1 + lad + 2 + lad + 3 * s + 1 + t, 1 + 7 + t + header_len, 1 + bits + 2 * lad + t + 3 * s


def row_elems(width: int, bits: int, header_len: int, blocks: int) -> int:
    _, inst, wit = shape(width, bits, header_len, blocks)
    return inst + wit


def _ladder(cs, a, d, point, b):
    r = (mu.select(cs, b[0], point[0], po.LC()), mu.select(cs, b[0], point[1], po.LC.const(1)))
    m = point
    for i in range(1, len(b)):
        m = ec.double(cs, a, m)
        t = ec.add(cs, a, d, r, m)
        r = (mu.select(cs, b[i], t[0], r[0]), mu.select(cs, b[i], t[1], r[1]))
    return r


def hybrid_circuit(curve, initial_state, generator, esk: int, pk, header, plaintext, bits: int, public=None, bit_values=None) -> po.R1CS:
    """public: (epk, tag, flat ciphertext) of the instance (default: the model's encryption); bit_values: the values of the Boolean witnesses (default: the bits
    of esk) -- both for negative tests"""
    fq, a, d, l = eu.params(curve)
    width = len(initial_state)
    rate = width - 1
    assert 1 <= bits <= l.bit_length() and 0 <= esk < min(l, 1 << bits) and all(len(blk) == rate for blk in plaintext)
    cs = po.R1CS(curve.fr)
    p = cs.f.p
    if public is None:
        epk, ct, tag = eu.hybrid_encrypt(curve, initial_state, generator, esk, pk, header, plaintext)
        public = (epk, tag, [v for blk in ct for v in blk])
    g = (cs.new_public(generator[0]), cs.new_public(generator[1]))
    pkv = (cs.new_public(pk[0]), cs.new_public(pk[1]))
    epk_pub = (cs.new_public(public[0][0]), cs.new_public(public[0][1]))
    tag_pub = cs.new_public(public[1])
    ct_pub = [cs.new_public(v) for v in public[2]]
    hv = [cs.new_public(v) for v in header]
    s = cs.new_witness(esk)
    vals = [(esk >> i) & 1 for i in range(bits)] if bit_values is None else list(bit_values)
    b = [mu.new_boolean_witness(cs, v) for v in vals]
    total = po.LC()
    for i, bi in enumerate(b):
        total = total.add(bi.scale(1 << i, p), p)
    cs.enforce(total, po.LC.const(1), s)
    e = _ladder(cs, a, d, g, b)
    cs.enforce(e[0], po.LC.const(1), epk_pub[0])
    cs.enforce(e[1], po.LC.const(1), epk_pub[1])
    key = list(_ladder(cs, a, d, pkv, b))
    pv = [[cs.new_witness(v) for v in blk] for blk in plaintext]
    state = [po.LC.const(v % p) for v in initial_state]
    for src in (key, hv):
        for k in range(len(src) // rate + 1):
            blk = src[k * rate:(k + 1) * rate]
            state = du.permute_gadget(cs, curve, [state[0]] + [state[1 + i].add(blk[i], p) if i < len(blk) else state[1 + i] for i in range(rate)])
    cts = []
    for blk in pv:
        c = [state[1 + i].add(blk[i], p) for i in range(rate)]
        cts += c
        state = du.permute_gadget(cs, curve, [state[0]] + c)
    cs.enforce(state[1], po.LC.const(1), tag_pub)
    for c, v in zip(cts, ct_pub):
        cs.enforce(c, po.LC.const(1), v)
    assert (cs.n_constraints, cs.n_instance, cs.n_witness) == shape(width, bits, len(header), len(plaintext))
    return cs


def item(curve, shape_whn, bits: int, seed: int, esk=None, pk=None):
    """(initial_state, G, esk, sk, pk, header, plaintext blocks) of one message at (W; H, N): G in the prime-order subgroup, pk = sk G"""
    width, h, n = shape_whn
    rate = width - 1
    l = eu.params(curve)[3]
    st = pu.random_elems(curve, width, seed)
    g = eu.subgroup_points(curve, 1, seed + 1)[0]
    sk = eu.random_scalars(curve, 1, seed + 2)[0]
    if esk is None:
        esk = eu.random_scalars(curve, 1, seed + 3)[0] % min(l, 1 << bits)
    vals = pu.random_elems(curve, h + n * rate, seed + 4)
    return st, g, esk, sk, (eu.mul(curve, sk, g) if pk is None else pk), vals[:h], [vals[h + j * rate:h + (j + 1) * rate] for j in range(n)]


def words(items, width):
    """items of one shape -> dict of the uint64 operands of the batched calls (one initial state and one generator: the first item's)"""
    count = len(items)
    h = len(items[0][5])
    return dict(st=pu.limbs(items[0][0]), g=eu.point_words([items[0][1]])[0], esk=pu.limbs([it[2] for it in items]), pk=eu.point_words([it[4] for it in items]),
                h=pu.limbs([v for it in items for v in it[5]]).reshape(count, h, 4), t=du.text_words([it[6] for it in items], width))
