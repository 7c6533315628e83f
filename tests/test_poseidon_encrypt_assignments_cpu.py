"""The host mirror behind zl_poseidon_encrypt_assignments (ctx == NULL: host_encrypt_assignments in csrc/zl_poseidon_dev.hip) against the assignments both host
compilers export and the independent Python builder of tests/poseidon_duplex_util.py, on both curves at widths 3..6; the row size; the tag and ciphertext
cells against the cipher's host mirror; the argument errors; and the shape coincidence the header states.  Shapes (K, H, N), rate = W - 1:
    A (1, 0, 1)         rate - 1 folded lanes, the empty header's one zero block
    B (rate, 0, 1)      nothing folded, the key's extra all-zero block: a permutation that absorbs nothing and records every S-box
    C (rate + 1, 1, 2)  two key blocks, a partial header, two message blocks
    F (2, rate, 1)      an exact header block and its zero block; rate - 2 folded lanes from width 4
    E (2, 0, 1)         width 4 only, the reference test's shape
Initial states: zero (NULL), a random one, and one whose rate lanes are non-zero constants (a folded lane then carries a non-zero value).  No GPU."""
import numpy as np
import pytest

import oracle_lib as ol
import poseidon_duplex_util as du
import poseidon_util as pu
from openzl_amd import Circuit, load_library, poseidon_duplex_encrypt_host, poseidon_encrypt_assignment_elems, poseidon_encrypt_assignments_host

CURVES = pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
WIDTHS = pytest.mark.parametrize("width", [3, 4, 5, 6])
EINVAL = -1


def shapes(width):
    rate = width - 1
    out = {"A": (1, 0, 1), "B": (rate, 0, 1), "C": (rate + 1, 1, 2), "F": (2, rate, 1)}
    if width == 4:
        out["E"] = (2, 0, 1)
    return out


def initial_states(curve, width):
    """name -> W integers, or None for the zero state"""
    return {"zero": None, "random": pu.random_elems(curve, width, 900 + width), "rate": [0] + [curve.fr.p - 1 - i for i in range(width - 1)]}


def witness_assignment(make):
    w = make()
    try:
        return w.arrays()["assignment"]
    finally:
        w.close()


def test_row_sizes():
    for width in (3, 4, 5, 6):
        for k, h, n in list(shapes(width).values()) + [(64, 64, 1024), (1, 64, 3), (64, 0, 1)]:
            n_c, n_i, n_w = du.circuit_shape(width, k, h, n)
            assert poseidon_encrypt_assignment_elems(width, k, h, n) == n_i + n_w, (width, k, h, n)
    assert poseidon_encrypt_assignment_elems(3, 2, 0, 1) == 953 and poseidon_encrypt_assignment_elems(6, 2, 0, 1) == 938
    for bad in ((2, 2, 0, 1), (7, 2, 0, 1), (3, 0, 0, 1), (3, 65, 0, 1), (3, 2, 65, 1), (3, 2, 0, 0), (3, 2, 0, 1025), (0, 1, 0, 1), (3, 1 << 40, 0, 1), (3, 1, 1 << 40, 1),
                (3, 1, 0, 1 << 40), (-1, 1, 0, 1)):
        assert poseidon_encrypt_assignment_elems(*bad) == 0, bad


@CURVES
@WIDTHS
def test_rows_equal_the_compilers_assignments(curve, width):
    rate = width - 1
    for si, (sname, st) in enumerate(initial_states(curve, width).items()):
        stw = None if st is None else pu.limbs(st)
        for name, shape in sorted(shapes(width).items()):
            k, h, n = shape
            assert poseidon_encrypt_assignments_host(curve.cid, stw, *(v[:0] for v in du.pack([], width, shape))).shape[0] == 0  # count 0 is accepted
            items = du.random_items(curve, width, shape, 40, 31 * width + si) + du.bound_items(curve, width, shape)  # more than one block of the host pool
            keys, headers, texts = du.pack(items, width, shape)
            rows = poseidon_encrypt_assignments_host(curve.cid, stw, keys, headers, texts)
            n_c, n_i, n_w = du.circuit_shape(width, k, h, n)
            what = (sname, name)
            assert rows.shape == (len(items), n_i + n_w, 4) == (len(items), poseidon_encrypt_assignment_elems(width, k, h, n), 4), what
            cts, tags = poseidon_duplex_encrypt_host(curve.cid, stw, keys, headers, texts)
            assert np.array_equal(rows[:, 0], np.tile(np.array([1, 0, 0, 0], dtype=np.uint64), (len(items), 1))), what
            assert np.array_equal(rows[:, 1], tags), what
            assert np.array_equal(rows[:, 2:2 + n * rate], cts.reshape(len(items), n * rate, 4)), what
            at = 2 + n * rate
            assert np.array_equal(rows[:, at:at + h], headers) and np.array_equal(rows[:, at + h:at + h + k], keys), what
            assert np.array_equal(rows[:, at + h + k:at + h + k + n * rate], texts.reshape(len(items), n * rate, 4)), what
            for j, (key, header, text) in enumerate(items):
                got = witness_assignment(lambda: Circuit.poseidon_encrypt(curve.cid, st, key, header, text, witness_only=True))
                assert np.array_equal(rows[j], got), (what, j)
            if si != sorted(shapes(width)).index(name) % 3:  # the full compiler and the Python builder: one row per shape, the states in turn
                continue
            j = 1 + si
            key, header, text = items[j]
            full = Circuit.poseidon_encrypt(curve.cid, st, key, header, text)
            try:
                assert full.shape == (n_c, n_i, n_w) and np.array_equal(rows[j], full.arrays()["assignment"]), what
            finally:
                full.close()
            j = 5 + si
            key, header, text = items[j]
            cs = du.encrypt_circuit(curve.fr, st if st is not None else [0] * width, key, header, text)
            assert np.array_equal(rows[j], ol.ints_to_limbs(cs.assignment(), 4)), what


@CURVES
def test_argument_errors(curve):
    L = load_library()
    r, p64 = curve.fr.p, ol.p64
    width, k, h, n = 3, 2, 1, 1
    st, key, hdr, text = pu.limbs([1, 2, 3]), pu.limbs([4, 5]), pu.limbs([8]), pu.limbs([6, 7])
    nv = poseidon_encrypt_assignment_elems(width, k, h, n)
    out = np.full((1, nv, 4), 0xA5, dtype=np.uint64)
    fn = L.zl_poseidon_encrypt_assignments
    for w in (2, 7):
        assert fn(None, curve.cid, w, p64(st), p64(key), k, p64(hdr), h, p64(text), n, 1, p64(out)) == EINVAL
    for kk in (0, 65):
        assert fn(None, curve.cid, width, p64(st), p64(pu.limbs([1] * 65)), kk, p64(hdr), h, p64(text), n, 1, p64(out)) == EINVAL
    assert fn(None, curve.cid, width, p64(st), p64(key), k, p64(pu.limbs([1] * 65)), 65, p64(text), n, 1, p64(out)) == EINVAL
    for nn in (0, 1025):
        assert fn(None, curve.cid, width, p64(st), p64(key), k, p64(hdr), h, p64(pu.limbs([1] * 2050)), nn, 1, p64(out)) == EINVAL
    assert fn(None, 77, width, p64(st), p64(key), k, p64(hdr), h, p64(text), n, 1, p64(out)) == EINVAL
    for args in ((None, p64(hdr), p64(text), p64(out)), (p64(key), None, p64(text), p64(out)), (p64(key), p64(hdr), None, p64(out)), (p64(key), p64(hdr), p64(text), None)):
        assert fn(None, curve.cid, width, p64(st), args[0], k, args[1], h, args[2], n, 1, args[3]) == EINVAL
    assert (out == 0xA5).all()
    for which in range(4):  # an element equal to r: initial state, key, header, plaintext
        for v in (r, (1 << 256) - 1):
            ops = [st.copy(), key.copy(), hdr.copy(), text.copy()]
            ops[which][-1] = pu.limbs([v])[0]
            assert fn(None, curve.cid, width, p64(ops[0]), p64(ops[1]), k, p64(ops[2]), h, p64(ops[3]), n, 1, p64(out.copy())) == EINVAL, which
    # count 0 is accepted and writes nothing; a NULL header pointer is accepted when header_len is 0; NULL initial_state is the zero state
    assert fn(None, curve.cid, width, p64(st), None, k, None, h, None, n, 0, None) == 0
    assert fn(None, curve.cid, width, p64(st), p64(key), k, p64(hdr), h, p64(text), n, 0, p64(out)) == 0 and (out == 0xA5).all()
    assert fn(None, curve.cid, width, p64(st), p64(key), k, p64(hdr), h, p64(text), n, 1, p64(out)) == 0 and (out[0, 0] == [1, 0, 0, 0]).all()
    out0 = np.zeros((1, poseidon_encrypt_assignment_elems(width, k, 0, n), 4), dtype=np.uint64)
    assert fn(None, curve.cid, width, None, p64(key), k, None, 0, p64(text), n, 1, p64(out0)) == 0
    assert np.array_equal(out0[0], witness_assignment(lambda: Circuit.poseidon_encrypt(curve.cid, None, [4, 5], [], [[6, 7]], witness_only=True)))
    # the device-pointer form never takes the host path: a null ctx is refused
    assert L.zl_poseidon_encrypt_assignments_dev(None, curve.cid, width, p64(st), p64(key), k, p64(hdr), h, p64(text), n, 1, p64(out), nv) == EINVAL


def test_one_pair_of_parameter_tuples_shares_a_shape():
    """the header's note: within the limits exactly (W, K, H, N) = (5, 15, 15, 5) and (6, 15, 15, 4) have one circuit shape"""
    # K, H, N rate and S are fixed by the shape (K = n_witness - n_constraints + 1, ...), so two tuples of one shape differ in the width
    ks, hs = np.arange(1, 65)[:, None, None], np.arange(0, 65)[None, :, None]

    def sboxes(w, n):
        rate, f = w - 1, du.sboxes(w)
        return f - 1 - np.maximum(0, rate - ks) + (ks // rate + 1 + hs // rate + 1 + n[None, None, :] - 1) * f

    pairs = []
    for w in (3, 4, 5, 6):
        for w2 in range(w + 1, 7):
            n = np.arange(1, 1025)
            ok = (n * (w - 1) % (w2 - 1) == 0) & (n * (w - 1) // (w2 - 1) <= 1024)
            n1, n2 = n[ok], (n * (w - 1) // (w2 - 1))[ok]
            for k, h, i in np.argwhere(sboxes(w, n1) == sboxes(w2, n2)):
                pairs.append(((w, int(k) + 1, int(h), int(n1[i])), (w2, int(k) + 1, int(h), int(n2[i]))))
    assert pairs == [((5, 15, 15, 5), (6, 15, 15, 4))]
    assert du.circuit_shape(5, 15, 15, 5) == du.circuit_shape(6, 15, 15, 4)
