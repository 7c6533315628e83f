"""Python model of Poseidon at every arity of the specification table (include/zl_backend_ext.h: zl_poseidon_spec): arity 2, 3, 4, 5 = width 3, 4, 5, 6 with
8 full and 55, 55, 56, 56 partial rounds and the domain tag 2^arity - 1.  The LFSR constants and the Cauchy matrix are generated ONCE per (curve, width)
(po.poseidon_permute regenerates them on every call); plain Python integers, in the style of tests/poseidon_util.py.  Pinned by
tests/test_poseidon_arity_host.py against po.poseidon_permute on one state per (curve, width)."""
import functools

import poseidon_util as pu
from oracle_lib import po

CURVES = pu.CURVES
ARITIES = [2, 3, 4, 5]
WIDTHS = [3, 4, 5, 6]
# arity -> (width, full rounds, partial rounds, tag)
SPEC = {2: (3, 8, 55, 3), 3: (4, 8, 55, 7), 4: (5, 8, 56, 15), 5: (6, 8, 56, 31)}


def rounds(width):
    _, rf, rp, _ = SPEC[width - 1]
    return rf, rp


@functools.lru_cache(maxsize=None)
def constants(curve_name: str, width: int):
    curve = {c.name: c for c in CURVES}[curve_name]
    rf, rp = rounds(width)
    return po.poseidon_round_constants(curve.fr, width, rf, rp), po.poseidon_mds(curve.fr, width)


def permute(curve, state):
    """the permutation of the width len(state): add round keys, x^5 on every lane in the first and last rf / 2 rounds and on lane 0 in between, full MDS"""
    w = len(state)
    keys, mds = constants(curve.name, w)
    rf, rp = rounds(w)
    p = curve.fr.p
    s = [v % p for v in state]
    half = rf // 2
    for rnd in range(rf + rp):
        s = [(v + keys[w * rnd + i]) % p for i, v in enumerate(s)]
        if rnd < half or rnd >= half + rp:
            s = [pow(v, 5, p) for v in s]
        else:
            s[0] = pow(s[0], 5, p)
        s = [sum(m * v for m, v in zip(row, s)) % p for row in mds]
    return s


def hash(curve, xs):
    """the hash of len(xs) inputs: element 0 of permute([2^arity - 1, x_1 .. x_arity])"""
    return permute(curve, [(1 << len(xs)) - 1] + list(xs))[0]


def edge_states(curve, width):
    """0, 1 and r - 1 in every position of a small base state, then the bound cases: all r - 1, all 0, and r - 1 in exactly one position of a zero state"""
    r = curve.fr.p
    base = [3, 7, 11, 13, 17, 19][:width]
    out = []
    for pos in range(width):
        for v in (0, 1, r - 1):
            st = list(base)
            st[pos] = v
            out.append(st)
    out.append([r - 1] * width)
    out.append([0] * width)
    for pos in range(width):
        st = [0] * width
        st[pos] = r - 1
        out.append(st)
    return out
