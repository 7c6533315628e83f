"""The duplex-encryption circuit of the host compilers (poseidon_encrypt in csrc/zl_host.hip over poseidon::permute of csrc/zl_host.h) against the independent
Python builder of tests/poseidon_duplex_util.py, array for array: CSR matrices and assignment of the full compiler, the assignment of the witness-only
compiler, the shape formula of the header, satisfaction and its loss when one public ciphertext element changes, and ZL_EINVAL for an empty key.  BLS12-381 at
widths 3..6, BN254 at width 3; shapes A, B, C (and E at width 4).  No GPU."""
import ctypes as C

import numpy as np
import pytest

import groth16_util as gu
import oracle_lib as ol
import poseidon_duplex_util as du
import poseidon_util as pu
from oracle_lib import po
from openzl_amd import BackendError, Circuit, load_library

EINVAL = -1
CASES = [(po.BLS12_381, w) for w in (3, 4, 5, 6)] + [(po.BN254, 3)]
CASE = pytest.mark.parametrize("curve,width", CASES, ids=lambda v: getattr(v, "name", str(v)))


def csr_satisfied(arrays, z, p) -> bool:
    prod = []
    for key in "ABC":
        ptr, col, val = arrays[key]
        vals = ol.limbs_to_ints(val) if len(col) else []
        prod.append([sum(vals[t] * z[int(col[t])] for t in range(int(ptr[i]), int(ptr[i + 1]))) % p for i in range(arrays["n_constraints"])])
    return all(a * b % p == c for a, b, c in zip(*prod))


def same_arrays(got, exp):
    return all(np.array_equal(g, e) for key in "ABC" for g, e in zip(got[key], exp[key]))


def test_shape_formula_examples():
    assert du.circuit_shape(3, 2, 0, 1) == (948, 4, 949)
    assert du.circuit_shape(6, 6, 1, 2) == (1568, 13, 1573)


@CASE
def test_compilers_build_the_python_builders_circuit(curve, width):
    p = curve.fr.p
    st = pu.random_elems(curve, width, 300 + width)
    for name, shape in sorted(du.shapes(width).items()):
        if name == "D":  # no key: not a circuit
            continue
        k, h, n = shape
        key, header, text = du.random_items(curve, width, shape, 1, 70 + width)[0]
        if name == "C":
            key[0], text[0][0], text[-1][-1] = p - 1, 0, p - 1
        cs = du.encrypt_circuit(curve.fr, st, key, header, text)
        z = ol.ints_to_limbs(cs.assignment(), 4)
        ct, tag = du.encrypt(curve, st, key, header, text)
        assert cs.is_satisfied() and cs.assignment()[1:2 + n * (width - 1) + h] == [tag] + [v for b in ct for v in b] + header
        full = Circuit.poseidon_encrypt(curve.cid, st, key, header, text)
        wit = Circuit.poseidon_encrypt(curve.cid, st, key, header, text, witness_only=True)
        try:
            assert full.shape == (cs.n_constraints, cs.n_instance, cs.n_witness) == du.circuit_shape(width, k, h, n), name
            assert cs.n_instance >= 4
            assert full.is_satisfied() and wit.is_satisfied()
            got = full.arrays()
            assert same_arrays(got, gu.r1cs_arrays(cs)), name
            assert np.array_equal(got["assignment"], z), name
            wa = wit.arrays()
            assert (wa["n_constraints"], wa["n_instance"], wa["n_witness"]) == (0, cs.n_instance, cs.n_witness)
            assert np.array_equal(wa["assignment"], got["assignment"]), name
            if name == "C":  # one changed public ciphertext element (the first, the last), the tag, a header element: not satisfied
                zi = cs.assignment()
                assert csr_satisfied(got, zi, p)
                for at in (1, 2, 1 + n * (width - 1), 2 + n * (width - 1)):
                    bad = list(zi)
                    bad[at] = (bad[at] + 1) % p
                    assert not csr_satisfied(got, bad, p), at
                public = [tag] + [v for b in ct for v in b]
                public[1] = (public[1] + 1) % p
                assert not du.encrypt_circuit(curve.fr, st, key, header, text, public=public).is_satisfied()
        finally:
            full.close()
            wit.close()


def test_zero_initial_state_is_the_null_pointer():
    curve, width = po.BLS12_381, 3
    key, header, text = du.random_items(curve, width, (2, 0, 1), 1, 5)[0]
    a = Circuit.poseidon_encrypt(curve.cid, None, key, header, text, witness_only=True)
    b = Circuit.poseidon_encrypt(curve.cid, [0, 0, 0], key, header, text, witness_only=True)
    try:
        assert np.array_equal(a.arrays()["assignment"], b.arrays()["assignment"])
        assert pu.ints(a.arrays()["assignment"][1])[0] == du.encrypt(curve, [0, 0, 0], key, header, text)[1]
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
def test_error_codes(curve):
    L = load_library()
    r, p64 = curve.fr.p, ol.p64
    st, key, text = pu.limbs([1, 2, 3]), pu.limbs([4, 5]), pu.limbs([6, 7])
    hdr = pu.limbs([8])
    for fn in (L.zl_circuit_poseidon_encrypt, L.zl_circuit_poseidon_encrypt_witness):
        h = C.c_void_p()
        assert fn(curve.cid, 3, p64(st), p64(key), 0, None, 0, p64(text), 1, C.byref(h)) == EINVAL  # key_len == 0
        assert fn(curve.cid, 3, p64(st), None, 2, None, 0, p64(text), 1, C.byref(h)) == EINVAL
        assert fn(curve.cid, 3, p64(st), p64(key), 2, None, 1, p64(text), 1, C.byref(h)) == EINVAL
        assert fn(curve.cid, 3, p64(st), p64(key), 2, None, 0, None, 1, C.byref(h)) == EINVAL
        assert fn(curve.cid, 3, p64(st), p64(key), 2, None, 0, p64(text), 1, None) == EINVAL
        assert fn(curve.cid, 3, p64(st), p64(key), 2, None, 0, p64(text), 0, C.byref(h)) == EINVAL
        assert fn(curve.cid, 2, p64(st), p64(key), 2, None, 0, p64(text), 1, C.byref(h)) == EINVAL
        assert fn(curve.cid, 7, p64(st), p64(key), 2, None, 0, p64(text), 1, C.byref(h)) == EINVAL
        assert fn(77, 3, p64(st), p64(key), 2, None, 0, p64(text), 1, C.byref(h)) == EINVAL
        for which in range(4):
            ops = [st.copy(), key.copy(), hdr.copy(), text.copy()]
            ops[which][-1] = pu.limbs([r])[0]
            assert fn(curve.cid, 3, p64(ops[0]), p64(ops[1]), 2, p64(ops[2]), 1, p64(ops[3]), 1, C.byref(h)) == EINVAL, which
        assert not h.value
        assert fn(curve.cid, 3, None, p64(key), 2, p64(hdr), 1, p64(text), 1, C.byref(h)) == 0 and h.value
        L.zl_circuit_free(h)
    for make in (lambda: Circuit.poseidon_encrypt(curve.cid, None, [], [], [[1, 2]]), lambda: Circuit.poseidon_encrypt(curve.cid, [1, 2], [1], [], [[1, 2]]),
                 lambda: Circuit.poseidon_encrypt(curve.cid, None, [r], [], [[1, 2]]), lambda: Circuit.poseidon_encrypt(curve.cid, None, [1], [], [[1, 2], [3]])):
        with pytest.raises(BackendError) as e:
            make()
        assert e.value.code == EINVAL
