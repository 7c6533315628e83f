"""Seeded generic R1CS circuits for the Groth16 tests (test infrastructure).  The Poseidon chain that every other proof test
uses has one shape only (two instance variables, one term per C row, no empty row, always satisfied); the circuits here
vary what that shape pins: the number of instance and witness variables, row lengths from empty to more than 64 terms,
boolean rows (A with one term, empty C), packing rows (a long C), degenerate coefficients and values, unsatisfied
assignments and domains that the constraints fill exactly.

generic_circuit() returns a po.R1CS, so csr(), assignment(), is_satisfied(), qap_witness_map() and the exponent
checks all apply unchanged; csr_edges() adds what an LC dict cannot express to the CSR arrays of groth16_util.r1cs_arrays."""
from __future__ import annotations

import random

import numpy as np

import oracle_lib as ol
from oracle_lib import po

KINDS = ("random", "empty", "boolean", "packing", "long")


def _coef(rng: random.Random, p: int) -> int:
    """a non-zero coefficient, weighted on 1 and r - 1"""
    u = rng.random()
    if u < 0.3:
        return 1
    if u < 0.5:
        return p - 1
    return rng.randrange(1, p)


def _value(rng: random.Random, p: int) -> int:
    """an assignment value, weighted on 0, 1 and r - 1"""
    u = rng.random()
    if u < 0.2:
        return 0
    if u < 0.4:
        return 1
    if u < 0.55:
        return p - 1
    return rng.randrange(p)


def _count(rng: random.Random, spec) -> int:
    return rng.randint(*spec) if isinstance(spec, tuple) else int(spec)


def generic_circuit(field: po.FieldParams, n_constraints: int, n_instance: int, n_witness: int, mix=None, terms=(3, 3, 3),
                    long_terms=(65, 90), pack_bits=8, satisfied: bool = True, seed: int = 0) -> po.R1CS:
    """A circuit of exactly (n_constraints, n_instance, n_witness).

    mix: {kind: weight} over KINDS (default: all rows random); row kinds are drawn with these weights.
      random  -- A, B, C with terms[0] / terms[1] / terms[2] terms (an int or an inclusive (lo, hi) range; 0 = empty)
      empty   -- A, B and C empty
      boolean -- x (x - 1) = 0: A = x, B = x - ONE, C empty
      packing -- v 1 = sum 2^i b_i: A = v, B = ONE, C = pack_bits terms over bit variables
      long    -- A (or B) with long_terms terms, the other one or two terms
    satisfied: every random / long row gets a slack witness of its own, only in that row's C with a non-zero coefficient, solved
    so that the row holds; bits are 0 / 1 and packed values their sums.  False: no slack witnesses, and every value is left as
    drawn (0, 1, r - 1 or uniform), so A z o B z - C z is non-zero on the domain."""
    p = field.p
    rng = random.Random(seed)
    mix = mix or {"random": 1}
    names = list(mix)
    kinds = rng.choices(names, weights=[mix[k] for k in names], k=n_constraints)
    assert all(k in KINDS for k in kinds), kinds
    n_bool, n_pack = kinds.count("boolean"), kinds.count("packing")
    n_slack = sum(1 for k in kinds if k in ("random", "long")) if satisfied else 0
    # the witness block: [free | bits | packed values | slack]; the free ones (and the instance block) feed random / long rows
    rest = n_witness - n_slack - n_pack
    n_bits = min(rest, max(n_bool, pack_bits * n_pack))
    if rest < 0 or n_bits < n_bool or (n_pack and n_bits < pack_bits):
        raise ValueError(f"n_witness = {n_witness} is too small for this row mix")
    n_free = rest - n_bits
    bits0, pv0, slack0 = n_free, n_free + n_bits, n_free + n_bits + n_pack

    cs = po.R1CS(field)
    for _ in range(n_instance - 1):
        cs.new_public(_value(rng, p))
    wit = [_value(rng, p) for _ in range(n_witness)]
    if satisfied:
        for j in range(bits0, pv0):
            wit[j] = rng.randrange(2)
    pool = [("i", j) for j in range(n_instance)] + [("w", j) for j in range(n_free)]

    def val(key):
        return cs.pub[key[1]] if key[0] == "i" else wit[key[1]]

    def lc(n):
        return po.LC({key: _coef(rng, p) for key in rng.sample(pool, min(n, len(pool)))})

    def lc_val(x: po.LC) -> int:
        return sum(c * val(key) for key, c in x.t.items()) % p

    bool_bits = list(range(bits0, bits0 + n_bool))
    slack, pv = slack0, pv0
    for kind in kinds:
        if kind == "empty":
            cs.enforce(po.LC(), po.LC(), po.LC())
            continue
        if kind == "boolean":
            x = ("w", bool_bits.pop())
            cs.enforce(po.LC({x: 1}), po.LC({x: 1, ("i", 0): p - 1}), po.LC())
            continue
        if kind == "packing":
            bits = rng.sample(range(bits0, pv0), pack_bits)
            c = po.LC({("w", b): pow(2, i, p) for i, b in enumerate(bits)})
            v = ("w", pv)
            pv += 1
            if satisfied:
                wit[v[1]] = lc_val(c)
            cs.enforce(po.LC({v: 1}), po.LC({("i", 0): 1}), c)
            continue
        if kind == "random":
            a, b, c = (lc(_count(rng, t)) for t in terms)
        else:  # long
            a, b = lc(_count(rng, long_terms)), lc(rng.randint(1, 2))
            if rng.random() < 0.5:
                a, b = b, a
            c = lc(rng.randint(0, 3))
        if satisfied:
            k, kc = ("w", slack), _coef(rng, p)
            slack += 1
            wit[k[1]] = (lc_val(a) * lc_val(b) - lc_val(c)) * pow(kc, -1, p) % p
            c.t[k] = kc
        cs.enforce(a, b, c)
    for v in wit:
        cs.wit.append(v)
    assert (cs.n_constraints, cs.n_instance, cs.n_witness) == (n_constraints, n_instance, n_witness)
    return cs


def csr_edges(arrays: dict, p: int, seed: int = 0) -> dict:
    """The same constraints in CSR forms an LC dict cannot hold: in every matrix, one row with an extra explicit zero coefficient, one
    row whose columns run in reverse order, and one term split into two entries of the same column whose coefficients add up to the
    original one.  Every row's value A_i z (B_i z, C_i z) is unchanged."""
    rng = random.Random(seed)
    nv = arrays["n_instance"] + arrays["n_witness"]
    out = dict(arrays)
    for key in "ABC":
        ptr, col, val = arrays[key]
        rows = []
        for i in range(len(ptr) - 1):
            rows.append([(int(col[k]), ol.limbs_to_ints(val[k:k + 1])[0]) for k in range(ptr[i], ptr[i + 1])])
        nonempty = [i for i, r in enumerate(rows) if r]
        multi = [i for i, r in enumerate(rows) if len(r) >= 2]
        if multi:
            rows[rng.choice(multi)].reverse()
        if nonempty:
            r = rows[rng.choice(nonempty)]
            j = rng.randrange(len(r))
            c, v = r[j]
            part = rng.randrange(1, p)
            r[j] = (c, part)
            r.insert(rng.randrange(len(r) + 1), (c, (v - part) % p))
        zero_row = rows[rng.randrange(len(rows))]
        zero_row.insert(rng.randrange(len(zero_row) + 1), (rng.randrange(nv), 0))
        new_ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
        flat = [t for r in rows for t in r]
        out[key] = (new_ptr, np.array([c for c, _ in flat], dtype=np.uint32), ol.ints_to_limbs([v for _, v in flat], 4))
    return out


def random_key_host(curve, nv: int, nw: int, nh: int, seed: int) -> dict:
    """A proving key of random points (known discrete logs, not a setup of any circuit) as host arrays, in the layout of
    groth16_util.setup_with_trapdoor: big enough for every circuit with at most nv variables, nw witnesses and N - 1 <= nh."""
    g1 = lambda n, s: ol.oracle_g1_mul_gen(curve, ol.random_scalars(curve, n, s))
    import groth16_util as gu

    single = ol.limbs_to_ints(ol.random_scalars(curve, 5, seed + 9))
    return {"a_query": g1(nv, seed + 1), "b_g1_query": g1(nv, seed + 2), "h_query": g1(nh, seed + 3), "l_query": g1(max(nw, 1), seed + 4),
            "b_g2_query": gu.g2_mul_gen(curve, ol.limbs_to_ints(ol.random_scalars(curve, nv, seed + 5))),
            "alpha_g1": g1(1, seed + 6)[0], "beta_g1": g1(1, seed + 7)[0], "delta_g1": g1(1, seed + 8)[0],
            "beta_g2": gu.g2_mul_gen(curve, single[:1])[0], "delta_g2": gu.g2_mul_gen(curve, single[1:2])[0]}


# The shape table of the generic-circuit tests (CPU: tests/test_r1cs_generic.py, device: tests/test_gpu_groth16_generic.py).
# name -> generic_circuit arguments; "edges" also goes through csr_edges.
SHAPES = {
    "smallest": dict(n_constraints=1, n_instance=1, n_witness=1),                          # N = 2: the transforms' smallest batch
    "full16": dict(n_constraints=13, n_instance=3, n_witness=20, mix={"random": 3, "boolean": 1}, terms=((1, 5), (1, 5), (0, 2))),  # instance tail ends on N - 1
    "full17": dict(n_constraints=14, n_instance=3, n_witness=20, mix={"random": 3, "boolean": 1}, terms=((1, 5), (1, 5), (0, 2))),  # one past: N = 32
    "many_publics": dict(n_constraints=5, n_instance=40, n_witness=7, terms=(5, 2, 1)),    # A tail (40) longer than the rows; eight-lane A
    "no_witness": dict(n_constraints=3, n_instance=2, n_witness=0, satisfied=False),        # empty l query
    "sparse_a": dict(n_constraints=200, n_instance=3, n_witness=240, mix={"boolean": 4, "random": 1}, terms=(1, (1, 3), (0, 2))),  # one-lane A with tail
    "long_c": dict(n_constraints=100, n_instance=3, n_witness=900, mix={"packing": 1}, pack_bits=12),  # eight-lane C
    "mixed": dict(n_constraints=300, n_instance=2, n_witness=300, mix={"empty": 2, "long": 1, "random": 1}),  # empty rows beside > 64 terms
    "edges": dict(n_constraints=20, n_instance=3, n_witness=40, terms=((0, 4), (1, 3), (0, 3))),  # + zero / unsorted / repeated CSR entries
    "unsat_sparse_a": dict(n_constraints=200, n_instance=3, n_witness=240, mix={"boolean": 4, "random": 1}, terms=(1, (1, 3), (0, 2)), satisfied=False),
    "unsat_mixed": dict(n_constraints=300, n_instance=2, n_witness=300, mix={"empty": 2, "long": 1, "random": 1}, satisfied=False),
}
# a key of random points big enough for every shape above
KEY_NV, KEY_NW, KEY_NH = 1024, 1024, 1023


def shape_case(curve, name: str, seed: int = 0):
    """(cs, arrays) for SHAPES[name] on `curve`: arrays = the CSR arrays handed to the provers"""
    import groth16_util as gu

    cs = generic_circuit(curve.fr, seed=seed + sum(map(ord, name)), **SHAPES[name])
    arrays = gu.r1cs_arrays(cs)
    if name == "edges":
        arrays = csr_edges(arrays, curve.fr.p, seed=seed)
    return cs, arrays
