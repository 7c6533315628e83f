"""Python model of the Poseidon duplex-sponge cipher (include/zl_backend_ext.h: zl_poseidon_duplex_*, zl_circuit_poseidon_encrypt), independent of the
library: plain Python integers over poseidon_arity_util.permute, and the circuit over the oracle's R1CS / LC with a width-general permutation gadget.
    setup blocks  chunks(key) then chunks(header), where chunks ALWAYS appends one last zero-padded chunk (also when nothing is left over);
    absorb        state[1 + i] += b[i], permute;  lane 0 is never written
    encrypt       state[1 + i] += p[i]; c[i] = state[1 + i] (read before the permutation); permute
    decrypt       p[i] = c[i] - state[1 + i]; state[1 + i] = c[i]; permute
    tag           state[1] after the last permutation"""
import poseidon_arity_util as pa
import poseidon_util as pu
from oracle_lib import po


def chunks(vals, rate):
    """padded_chunks_with(vals, rate, 0): len(vals) // rate + 1 chunks of exactly `rate` elements"""
    vals = list(vals)
    out = [vals[i:i + rate] for i in range(0, len(vals) - len(vals) % rate, rate)]
    last = vals[len(vals) - len(vals) % rate:]
    out.append(last + [0] * (rate - len(last)))
    assert len(out) == len(vals) // rate + 1 and all(len(c) == rate for c in out)
    return out


def setup_blocks(width, key_len, header_len):
    return key_len // (width - 1) + 1 + header_len // (width - 1) + 1


def permutations(width, key_len, header_len, blocks):
    return setup_blocks(width, key_len, header_len) + blocks


def _setup(curve, state, key, header):
    p, rate = curve.fr.p, len(state) - 1
    s = list(state)
    for b in chunks(key, rate) + chunks(header, rate):
        s = pa.permute(curve, [s[0]] + [(s[1 + i] + b[i]) % p for i in range(rate)])
    return s


def encrypt(curve, initial_state, key, header, plaintext):
    """plaintext: N blocks of W - 1 integers -> (ciphertext blocks, tag)"""
    p, rate = curve.fr.p, len(initial_state) - 1
    s = _setup(curve, initial_state, key, header)
    out = []
    for blk in plaintext:
        assert len(blk) == rate
        c = [(s[1 + i] + blk[i]) % p for i in range(rate)]
        out.append(c)
        s = pa.permute(curve, [s[0]] + c)
    return out, s[1]


def decrypt(curve, initial_state, key, header, ciphertext, tag):
    """-> (plaintext blocks, whether `tag` is the computed tag)"""
    p, rate = curve.fr.p, len(initial_state) - 1
    s = _setup(curve, initial_state, key, header)
    out = []
    for blk in ciphertext:
        out.append([(blk[i] - s[1 + i]) % p for i in range(rate)])
        s = pa.permute(curve, [s[0]] + list(blk))
    return out, s[1] == tag


# ---- in circuit ------------------------------------------------------------------------------------------------------------------------------------------
def sboxes(width):
    """F: the S-boxes of one permutation"""
    rf, rp = pa.rounds(width)
    return rf * width + rp


def circuit_shape(width, key_len, header_len, blocks):
    """(n_constraints, n_instance, n_witness) as the header states it"""
    rate = width - 1
    f = sboxes(width)
    s = (f - 1 - max(0, rate - key_len)) + (permutations(width, key_len, header_len, blocks) - 1) * f
    return 3 * s + 1 + blocks * rate, 2 + blocks * rate + header_len, key_len + blocks * rate + 3 * s


def permute_gadget(cs: po.R1CS, curve, state):
    """the permutation on len(state) linear combinations; cs.mul folds an S-box whose input is a constant"""
    p = cs.f.p
    t = len(state)
    keys, mds = pa.constants(curve.name, t)
    rf, rp = pa.rounds(t)
    half = rf // 2
    state = list(state)
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
    return state


def encrypt_circuit(field, initial_state, key, header, plaintext, public=None) -> po.R1CS:
    """public: the [tag] + ciphertext values of the instance (default: the encryption's) -- for negative tests"""
    curve = {c.fr.p: c for c in pu.CURVES}[field.p]
    p, width = field.p, len(initial_state)
    rate = width - 1
    assert len(key) >= 1 and all(len(b) == rate for b in plaintext)
    cs = po.R1CS(field)
    if public is None:
        ct, tag = encrypt(curve, initial_state, key, header, plaintext)
        public = [tag] + [v for b in ct for v in b]
    pub = [cs.new_public(v) for v in public]
    hv = [cs.new_public(v) for v in header]
    kv = [cs.new_witness(v) for v in key]
    pv = [[cs.new_witness(v) for v in b] for b in plaintext]
    state = [po.LC.const(v % p) for v in initial_state]
    for src in (kv, hv):
        for b in range(len(src) // rate + 1):
            blk = src[b * rate:(b + 1) * rate]  # the padding zeros add nothing
            state = permute_gadget(cs, curve, [state[0]] + [state[1 + i].add(blk[i], p) if i < len(blk) else state[1 + i] for i in range(rate)])
    cts = []
    for blk in pv:
        c = [state[1 + i].add(blk[i], p) for i in range(rate)]
        cts += c
        state = permute_gadget(cs, curve, [state[0]] + c)
    cs.enforce(state[1], po.LC.const(1), pub[0])
    for c, v in zip(cts, pub[1:]):
        cs.enforce(c, po.LC.const(1), v)
    assert (cs.n_constraints, cs.n_instance, cs.n_witness) == circuit_shape(width, len(key), len(header), len(plaintext))
    return cs


# ---- shapes and data of the tests --------------------------------------------------------------------------------------------------------------------------
def shapes(width):
    """name -> (K, H, N): A minimal (partial key block, empty header); B an exact key block and its extra zero block; C two key blocks, a partial header, two
    message blocks; D no key and an exact header; E the reference test's shape (width 4 only)"""
    rate = width - 1
    out = {"A": (1, 0, 1), "B": (rate, 0, 1), "C": (rate + 1, 1, 2), "D": (0, rate, 3)}
    if width == 4:
        out["E"] = (2, 0, 1)
    return out


def bound_items(curve, width, shape):
    """the bound cases of a shape as (key, header, plaintext blocks): key / header / plaintext all r - 1, all of them together, all zero"""
    k, h, n = shape
    m, rate = curve.fr.p - 1, width - 1
    text = lambda v: [[v] * rate for _ in range(n)]
    return [([m] * k, [1] * h, text(2)), ([3] * k, [m] * h, text(4)), ([5] * k, [6] * h, text(m)), ([m] * k, [m] * h, text(m)), ([0] * k, [0] * h, text(0))]


def random_items(curve, width, shape, count, seed):
    k, h, n = shape
    rate = width - 1
    per = k + h + n * rate
    vals = pu.random_elems(curve, per * count, seed)
    out = []
    for i in range(count):
        v = vals[per * i:per * (i + 1)]
        out.append((v[:k], v[k:k + h], [v[k + h + rate * j:k + h + rate * (j + 1)] for j in range(n)]))
    return out


def pack(items, width, shape):
    """items -> (keys (count, K, 4), headers (count, H, 4), texts (count, N, W - 1, 4)) uint64 words"""
    k, h, n = shape
    count = len(items)
    keys = pu.limbs([v for it in items for v in it[0]]).reshape(count, k, 4)
    headers = pu.limbs([v for it in items for v in it[1]]).reshape(count, h, 4)
    texts = pu.limbs([v for it in items for b in it[2] for v in b]).reshape(count, n, width - 1, 4)
    return keys, headers, texts


def text_words(blocks_per_item, width):
    """[[block, ...], ...] -> (count, N, W - 1, 4) words"""
    count = len(blocks_per_item)
    return pu.limbs([v for blocks in blocks_per_item for b in blocks for v in b]).reshape(count, -1, width - 1, 4)
