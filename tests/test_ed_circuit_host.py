"""The scalar-multiplication circuit of the host compilers (ed_scalar_mul_circuit in csrc/zl_host.hip over the gadget of csrc/zl_host.h, namespace edwards)
against the independent Python builder of tests/ed_circuit_util.py, word for word: CSR matrices and assignment of the full compiler, the assignment of the
witness-only compiler, the host mirror of the device trace (zl_ed_scalar_mul_assignments with a NULL ctx), the shape formula, satisfaction and its loss when a
bit witness or a coordinate of Q changes, every ZL_EINVAL of the header, the arithmetic that keeps this family's shape apart from an encryption's, and one
proof at bits = 5 by the CPU prover over the library's matrices and row.  Both curves at bits 1, 2, 5 and full width.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import ed_circuit_util as ec
import edwards_util as eu
import groth16_util as gu
import oracle_lib as ol
import poseidon_duplex_util as du
import poseidon_util as pu
from oracle_lib import po
from openzl_amd import BackendError, Circuit, ed_order_bits, ed_scalar_mul_assignment_elems, ed_scalar_mul_assignments_host, load_library

EINVAL = -1
CURVE = pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
TD = po.Groth16Trapdoor(alpha=0x1357_2468_9ABC, beta=0x2222_3333_4444, gamma=0x5555_6666, delta=0x7777_8888_9999, tau=0xAAAA_BBBB_CCCC_D001)
R_, S_ = 0x1234_5678_9ABC_DEF0_3333, 0x0FED_CBA9_8765_4321_4444


def bit_widths(curve):
    return [1, 2, 5, ec.full_bits(curve)]


def points(curve):
    """the identity, a point of order 8, a point of the prime-order subgroup, a point of the full group"""
    return [eu.ID, eu.small_order_points(curve)[2], eu.subgroup_points(curve, 1, 21)[0], eu.random_points(curve, 1, 22)[0]]


def scalars(curve, bits):
    l = eu.params(curve)[3]
    top = l - 1 if bits == l.bit_length() else (1 << bits) - 1
    mid = eu.random_scalars(curve, 1, 23 + bits)[0] % (top + 1)
    return sorted({0, 1, top, mid})


def csr_satisfied(arrays, z, p) -> bool:
    prod = []
    for key in "ABC":
        ptr, col, val = arrays[key]
        vals = ol.limbs_to_ints(val) if len(col) else []
        prod.append([sum(vals[t] * z[int(col[t])] for t in range(int(ptr[i]), int(ptr[i + 1]))) % p for i in range(arrays["n_constraints"])])
    return all(a * b % p == c for a, b, c in zip(*prod))


def same_arrays(got, exp):
    return all(np.array_equal(g, e) for key in "ABC" for g, e in zip(got[key], exp[key]))


@CURVE
def test_full_widths_and_shape_formula(curve):
    full = {"bls12_381": 252, "bn254": 251}[curve.name]
    assert ec.full_bits(curve) == ed_order_bits(curve.cid) == full
    assert ec.shape(full)[0] == {252: 3520, 251: 3506}[full]
    for bits in range(1, full + 1):
        assert ed_scalar_mul_assignment_elems(curve.cid, bits) == 14 * bits - 5 == ec.shape(bits)[1] + ec.shape(bits)[2]
    for bits in (0, full + 1, 256, 2**31):
        assert ed_scalar_mul_assignment_elems(curve.cid, bits) == 0
    assert ed_scalar_mul_assignment_elems(77, 5) == 0


@CURVE
def test_compilers_build_the_python_builders_circuit(curve):
    for bits in bit_widths(curve):
        for i, pt in enumerate(points(curve)):
            ks = scalars(curve, bits)
            for k in ks if i == 2 or bits <= 5 else ks[-1:]:  # (at full width every scalar on the subgroup point, the largest on the others)
                cs = ec.scalar_mul_circuit(curve, bits, pt, k)
                z = cs.assignment()
                assert cs.is_satisfied() and tuple(z[1:5]) == pt + eu.mul(curve, k, pt) and z[5] == k
                full = Circuit.ed_scalar_mul(curve.cid, pt, k, bits)
                wit = Circuit.ed_scalar_mul(curve.cid, pt, k, bits, witness_only=True)
                try:
                    assert full.shape == (cs.n_constraints, cs.n_instance, cs.n_witness) == ec.shape(bits), (bits, pt, k)
                    assert full.is_satisfied() and wit.is_satisfied() and full.witness_only_compatible()
                    got = full.arrays()
                    assert same_arrays(got, gu.r1cs_arrays(cs)), (bits, pt, k)
                    assert np.array_equal(got["assignment"], ol.ints_to_limbs(z, 4)), (bits, pt, k)
                    wa = wit.arrays()
                    assert (wa["n_constraints"], wa["n_instance"], wa["n_witness"]) == (0, cs.n_instance, cs.n_witness)
                    assert np.array_equal(wa["assignment"], got["assignment"]), (bits, pt, k)
                finally:
                    full.close()
                    wit.close()


@CURVE
def test_default_width_is_the_full_width(curve):
    pt, k = points(curve)[2], eu.params(curve)[3] - 1
    a, b = Circuit.ed_scalar_mul(curve.cid, pt, k, witness_only=True), Circuit.ed_scalar_mul(curve.cid, pt, k, ec.full_bits(curve), witness_only=True)
    try:
        assert np.array_equal(a.arrays()["assignment"], b.arrays()["assignment"])
    finally:
        a.close()
        b.close()


@CURVE
def test_a_flipped_bit_or_a_changed_result_is_not_satisfied(curve):
    p = curve.fr.p
    for bits in (2, 5):
        pt, k = points(curve)[2], scalars(curve, bits)[-2]
        full = Circuit.ed_scalar_mul(curve.cid, pt, k, bits)
        try:
            got = full.arrays()
        finally:
            full.close()
        z = pu.ints(got["assignment"])
        assert csr_satisfied(got, z, p)
        for at in range(6, 6 + bits):  # one bit witness, the records left as they are
            bad = list(z)
            bad[at] ^= 1
            assert not csr_satisfied(got, bad, p), (bits, at)
        for at in (3, 4):  # one coordinate of Q
            bad = list(z)
            bad[at] = (bad[at] + 1) % p
            assert not csr_satisfied(got, bad, p), (bits, at)
        # the builder as a prover who flips a bit and follows it through every record: only the decomposition row and Q fail, and they do
        vals = [(k >> i) & 1 for i in range(bits)]
        vals[bits - 1] ^= 1
        assert not ec.scalar_mul_circuit(curve, bits, pt, k, bit_values=vals).is_satisfied()
        q = eu.mul(curve, k, pt)
        assert not ec.scalar_mul_circuit(curve, bits, pt, k, q=(q[0], (q[1] + 1) % p)).is_satisfied()
        assert not ec.scalar_mul_circuit(curve, bits, pt, k, q=eu.mul(curve, k + 1, pt)).is_satisfied()


@CURVE
def test_error_codes(curve):
    L = load_library()
    q, a, d, l = eu.params(curve)
    full = l.bit_length()
    pt = points(curve)[2]
    off = (pt[0], (pt[1] + 1) % q)
    assert not eu.on_curve(curve, off)
    P, k5 = eu.point_words([pt])[0], pu.limbs([19])
    for fn in (L.zl_circuit_ed_scalar_mul, L.zl_circuit_ed_scalar_mul_witness):
        h = C.c_void_p()
        call = lambda cid, bits, pw, kw: fn(cid, bits, ol.p64(np.ascontiguousarray(pw)), ol.p64(np.ascontiguousarray(kw)), C.byref(h))
        assert call(77, 5, P, k5) == EINVAL                                        # an unknown curve
        assert call(curve.cid, 0, P, k5) == EINVAL                                 # bits out of range
        assert call(curve.cid, full + 1, P, k5) == EINVAL
        assert call(curve.cid, 5, eu.point_words([(q, pt[1])])[0], k5) == EINVAL   # a coordinate >= q
        assert call(curve.cid, 5, eu.point_words([(pt[0], q + 1)])[0], k5) == EINVAL
        assert call(curve.cid, 5, eu.point_words([off])[0], k5) == EINVAL          # a point off the curve
        assert call(curve.cid, full, P, pu.limbs([l])) == EINVAL                   # a scalar >= l
        assert call(curve.cid, 5, P, pu.limbs([32])) == EINVAL                     # a scalar >= 2^bits
        assert call(curve.cid, 4, P, k5) == EINVAL
        assert call(curve.cid, 5, P, pu.limbs([1 << 200])) == EINVAL
        assert fn(curve.cid, 5, None, ol.p64(k5), C.byref(h)) == EINVAL
        assert fn(curve.cid, 5, ol.p64(P), None, C.byref(h)) == EINVAL
        assert fn(curve.cid, 5, ol.p64(P), ol.p64(k5), None) == EINVAL
        assert not h.value
        assert call(curve.cid, 5, P, k5) == 0 and h.value
        L.zl_circuit_free(h)
    assert L.zl_circuit_witness_only_compatible(None) == EINVAL
    for make in (lambda: Circuit.ed_scalar_mul(curve.cid, off, 3, 5), lambda: Circuit.ed_scalar_mul(curve.cid, pt, l, full), lambda: Circuit.ed_scalar_mul(curve.cid, pt, 32, 5),
                 lambda: Circuit.ed_scalar_mul(curve.cid, pt, 1, 0), lambda: Circuit.ed_scalar_mul(curve.cid, pt, -1, 5)):
        with pytest.raises(BackendError) as e:
            make()
        assert e.value.code == EINVAL
    # the host mirror of the trace refuses the same items, and the same parameters
    good = eu.point_words([pt, pt, pt])
    ks = pu.limbs([3, 5, 7])
    assert ed_scalar_mul_assignments_host(curve.cid, good, ks, 5).shape == (3, 65, 4)
    for pts_w, ks_w, bits in ((eu.point_words([pt, off, pt]), ks, 5), (eu.point_words([pt, pt, (q, 1)]), ks, 5), (good, pu.limbs([3, 32, 7]), 5),
                              (good, pu.limbs([3, 5, l]), full)):
        with pytest.raises(BackendError) as e:
            ed_scalar_mul_assignments_host(curve.cid, pts_w, ks_w, bits)
        assert e.value.code == EINVAL
    out = np.zeros((3, 65, 4), dtype=np.uint64)
    assert L.zl_ed_scalar_mul_assignments(None, curve.cid, 0, ol.p64(good), 1, ol.p64(ks), 3, ol.p64(out)) == EINVAL
    assert L.zl_ed_scalar_mul_assignments(None, curve.cid, full + 1, ol.p64(good), 1, ol.p64(ks), 3, ol.p64(out)) == EINVAL
    assert L.zl_ed_scalar_mul_assignments(None, 77, 5, ol.p64(good), 1, ol.p64(ks), 3, ol.p64(out)) == EINVAL
    assert L.zl_ed_scalar_mul_assignments(None, curve.cid, 5, ol.p64(good), 2, ol.p64(ks), 3, ol.p64(out)) == EINVAL
    assert L.zl_ed_scalar_mul_assignments(None, curve.cid, 5, None, 1, ol.p64(ks), 3, ol.p64(out)) == EINVAL
    assert L.zl_ed_scalar_mul_assignments(None, curve.cid, 5, ol.p64(good), 1, ol.p64(ks), 3, None) == EINVAL
    assert L.zl_ed_scalar_mul_assignments(None, curve.cid, 5, None, 1, None, 0, None) == 0
    assert L.zl_ed_scalar_mul_assignments_dev(None, curve.cid, 5, None, 1, None, 0, None, 65) == EINVAL  # the device form has no host path


@CURVE
def test_host_mirror_rows_are_the_compilers_assignment(curve):
    for bits in bit_widths(curve):
        pts = points(curve)
        ks = scalars(curve, bits)
        pairs = [(pt, k) for pt in pts for k in ks]
        rows = ed_scalar_mul_assignments_host(curve.cid, eu.point_words([pt for pt, _ in pairs]), pu.limbs([k for _, k in pairs]), bits)
        assert rows.shape == (len(pairs), 14 * bits - 5, 4)
        for row, (pt, k) in zip(rows, pairs):
            c = Circuit.ed_scalar_mul(curve.cid, pt, k, bits, witness_only=True)
            try:
                assert np.array_equal(row, c.arrays()["assignment"]), (bits, pt, k)
            finally:
                c.close()
        shared = ed_scalar_mul_assignments_host(curve.cid, eu.point_words([pts[3]])[0], pu.limbs(ks), bits)  # one point for all items
        per_item = [row for row, (pt, _) in zip(rows, pairs) if pt == pts[3]]
        assert np.array_equal(shared, np.stack(per_item))


def test_no_encryption_has_this_shape():
    """an encryption circuit's shape is (2 + N rate + H, K + N rate + 3 S, 3 S + 1 + N rate), so K = n_witness - (n_constraints - 1) >= 1; here that is -1"""
    for bits in (1, 2, 5, 251, 252):
        n_constraints, n_instance, n_witness = ec.shape(bits)
        assert n_instance == 5 and n_witness - (n_constraints - 1) == -1
    for width in (3, 4, 5, 6):
        for k, h, n in ((1, 0, 1), (2, 0, 1), (2, 1, 1), (1, 2, 1), (64, 64, 3)):
            rows, inst, wit = du.circuit_shape(width, k, h, n)
            assert wit - (rows - 1) == k >= 1
            assert inst != 5 or (rows, inst, wit) not in {ec.shape(b) for b in range(1, 253)}


@CURVE
def test_a_proof_of_five_bits_verifies_and_a_wrong_result_does_not(curve):
    """the CPU prover over the LIBRARY's matrices and the host mirror's row; the proof is the group element the trapdoor predicts, the Groth16 equation holds
    for the public inputs (P, Q) and fails for (P, Q') -- in the exponent, where the setup's discrete logs are known"""
    r = curve.fr.p
    bits, pt, k = 5, points(curve)[2], 21
    cs = ec.scalar_mul_circuit(curve, bits, pt, k)
    full = Circuit.ed_scalar_mul(curve.cid, pt, k, bits)
    try:
        arrays = full.arrays()
    finally:
        full.close()
    assert same_arrays(arrays, gu.r1cs_arrays(cs))
    row = ed_scalar_mul_assignments_host(curve.cid, eu.point_words([pt]), pu.limbs([k]), bits)[0]
    assert pu.ints(row) == cs.assignment()
    pk = gu.setup_with_trapdoor(curve, cs, TD)
    n = 1 << cs.domain_log()
    rs = ol.ints_to_limbs([R_, S_], 4)
    (a, ai, b, bi, c, ci), h = gu.oracle_prove(curve, arrays, np.ascontiguousarray(row), pk, rs[0], rs[1], threads=4, want_h=n)
    h_ints = ol.limbs_to_ints(h)
    assert h_ints == po.qap_witness_map(curve, cs) and h_ints[-1] == 0
    A, B, Cx = po.groth16_prove_exponents(curve, cs, TD, pk["ex"], h_ints, R_, S_)
    assert not (ai or bi or ci)
    assert (a == ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs([A], 4))[0]).all() and (b == gu.g2_mul_gen(curve, [B])[0]).all()
    assert (c == ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs([Cx], 4))[0]).all()

    def verifies(public):
        pub = sum(x * g for x, g in zip([1] + list(public), pk["ex"]["gamma_abc"])) % r
        return (A * B - TD.alpha * TD.beta - pub * TD.gamma - Cx * TD.delta) % r == 0

    q = eu.mul(curve, k, pt)
    assert verifies(pt + q) and po.groth16_check_exponents(curve, cs, TD, pk["ex"], A, B, Cx)
    assert not verifies(pt + (q[0], (q[1] + 1) % r))
    assert not verifies(pt + eu.mul(curve, k + 1, pt))
    assert not verifies(eu.mul(curve, 2, pt) + q)
