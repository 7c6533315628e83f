"""The Poseidon duplex cipher through its host path (ctx == NULL: poseidon::duplex_encrypt / duplex_decrypt of csrc/zl_host.h over the host pool) against the
Python model of tests/poseidon_duplex_util.py: both curves, widths 3..6, the shapes A..E of the model, the decryption round trip, the anchor to the reference's
permutation fixture, the permutation count, every ZL_EINVAL, count == 0 and the in-place call.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle_lib as ol
import poseidon_arity_util as pa
import poseidon_duplex_util as du
import poseidon_util as pu
from oracle_lib import po
from openzl_amd import BackendError, load_library
from openzl_amd import backend as zb

HERE = os.path.dirname(os.path.abspath(__file__))
FX = json.load(open(os.path.join(HERE, "golden", "ref_poseidon_fixtures.json")))
CURVES = pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
WIDTHS = pytest.mark.parametrize("width", pa.WIDTHS)
EINVAL = -1


def blocks_of(words):
    """(count, N, W - 1, 4) words -> [[block of ints, ...] per item]"""
    count, n, rate, _ = words.shape
    flat = pu.ints(words)
    return [[flat[(i * n + j) * rate:(i * n + j + 1) * rate] for j in range(n)] for i in range(count)]


def test_chunking_rule_always_appends_a_last_chunk():
    assert du.chunks([], 2) == [[0, 0]]
    assert du.chunks([7], 2) == [[7, 0]]
    assert du.chunks([7, 8], 2) == [[7, 8], [0, 0]]
    assert du.chunks([7, 8, 9], 2) == [[7, 8], [9, 0]]
    assert du.setup_blocks(3, 0, 0) == 2 and du.setup_blocks(3, 2, 0) == 3 and du.setup_blocks(6, 6, 1) == 3


@CURVES
@WIDTHS
def test_host_mirror_is_the_model_and_decrypts_back(curve, width):
    st = pu.random_elems(curve, width, 900 + width)
    for n_shape, (name, shape) in enumerate(sorted(du.shapes(width).items())):
        items = du.bound_items(curve, width, shape) + du.random_items(curve, width, shape, 3, 40 + width)
        keys, headers, texts = du.pack(items, width, shape)
        for init in (None, st) if n_shape == 0 else (st,):  # (the last one is st: the wrong-tag call below uses its results)
            init_ints = st if init is not None else [0] * width
            exp = [du.encrypt(curve, init_ints, *it) for it in items]
            ct, tags = zb.poseidon_duplex_encrypt_host(curve.cid, None if init is None else pu.limbs(init), keys, headers, texts)
            assert ct.shape == texts.shape and tags.shape == (len(items), 4)
            assert blocks_of(ct) == [e[0] for e in exp], name
            assert pu.ints(tags) == [e[1] for e in exp], name
            back, ok = zb.poseidon_duplex_decrypt_host(curve.cid, None if init is None else pu.limbs(init), keys, headers, ct, tags)
            assert ok.dtype == bool and ok.all() and back.tobytes() == texts.tobytes(), name
            assert [du.decrypt(curve, init_ints, it[0], it[1], e[0], e[1]) for it, e in zip(items, exp)] == [(it[2], True) for it in items]
        # a wrong tag is a verdict, not an error, and the plaintext is returned all the same
        bad = tags.copy()
        bad[1] = pu.limbs([(pu.ints(tags[1])[0] + 1) % curve.fr.p])[0]
        back, ok = zb.poseidon_duplex_decrypt_host(curve.cid, pu.limbs(st), keys, headers, ct, bad)
        assert list(ok) == [i != 1 for i in range(len(items))] and back.tobytes() == texts.tobytes()


def test_anchor_to_the_reference_permutation_fixture():
    """BLS12-381, width 3, [3, 1, 2], no key, no header, plaintext [0, 0]: the state after the first setup permutation is the reference's width-3 output"""
    curve = po.BLS12_381
    first = [int(v) for v in FX["permutation_width3"]["output"]]
    assert pa.permute(curve, [3, 1, 2]) == first
    second = pa.permute(curve, first)
    ct, tags = zb.poseidon_duplex_encrypt_host(curve.cid, pu.limbs([3, 1, 2]), np.zeros((1, 0, 4), np.uint64), np.zeros((1, 0, 4), np.uint64),
                                               np.zeros((1, 1, 2, 4), np.uint64))
    assert pu.ints(ct) == second[1:]
    assert pu.ints(tags) == [pa.permute(curve, second)[1]]
    assert du.encrypt(curve, [3, 1, 2], [], [], [[0, 0]]) == ([second[1:]], pa.permute(curve, second)[1])


def test_permutation_count():
    for width in pa.WIDTHS:
        for k, h, n in [(0, 0, 1), (1, 0, 1), (width - 1, 0, 1), (width, 1, 2), (0, width - 1, 3), (64, 64, 1024)]:
            assert zb.poseidon_duplex_permutations(width, k, h, n) == du.permutations(width, k, h, n) == k // (width - 1) + 1 + h // (width - 1) + 1 + n
    for bad in [(2, 1, 0, 1), (7, 1, 0, 1), (3, 65, 0, 1), (3, 0, 65, 1), (3, 1, 0, 0), (3, 1, 0, 1025)]:
        assert zb.poseidon_duplex_permutations(*bad) == 0


@CURVES
def test_error_codes_count_zero_and_in_place(curve):
    L = load_library()
    r, width, shape = curve.fr.p, 4, (4, 1, 2)
    items = du.random_items(curve, width, shape, 5, 11)
    keys, headers, texts = du.pack(items, width, shape)
    st = pu.limbs(pu.random_elems(curve, width, 12))
    ct, tags = zb.poseidon_duplex_encrypt_host(curve.cid, st, keys, headers, texts)
    p64, ok = ol.p64, np.zeros(5, dtype=np.uint8)
    okp = ok.ctypes.data_as(C.POINTER(C.c_uint8))
    out, tg = np.zeros_like(texts), np.zeros((5, 4), dtype=np.uint64)

    def enc(curve_id=curve.cid, w=width, s=p64(st), k=p64(keys), kl=4, h=p64(headers), hl=1, t=p64(texts), n=2, count=5, o=p64(out), g=p64(tg)):
        return L.zl_poseidon_duplex_encrypt_batch(None, curve_id, w, s, k, kl, h, hl, t, n, count, o, g)

    def dec(curve_id=curve.cid, w=width, s=p64(st), k=p64(keys), kl=4, h=p64(headers), hl=1, t=p64(ct), g=p64(tags), n=2, count=5, o=p64(out), v=okp):
        return L.zl_poseidon_duplex_decrypt_batch(None, curve_id, w, s, k, kl, h, hl, t, g, n, count, o, v)

    assert enc() == 0 and out.tobytes() == ct.tobytes() and tg.tobytes() == tags.tobytes()
    assert dec() == 0 and out.tobytes() == texts.tobytes() and ok.all()
    for fn in (enc, dec):
        assert fn(curve_id=77) == EINVAL
        for w in (0, 2, 7):
            assert fn(w=w) == EINVAL
        assert fn(kl=65) == EINVAL and fn(hl=65) == EINVAL
        assert fn(n=0) == EINVAL and fn(n=1025) == EINVAL
        assert fn(k=None) == EINVAL and fn(h=None) == EINVAL and fn(t=None) == EINVAL and fn(o=None) == EINVAL and fn(g=None) == EINVAL
        # count == 0: nothing is read or written, but the parameters are still checked
        before = (out.tobytes(), tg.tobytes())
        assert fn(count=0) == 0 and fn(count=0, k=None, h=None, t=None, o=None, g=None) == 0 and fn(count=0, w=7) == EINVAL
        assert (out.tobytes(), tg.tobytes()) == before
    assert dec(v=None) == EINVAL
    # keys may be NULL when key_len == 0, headers when header_len == 0
    assert enc(k=None, kl=0, h=None, hl=0) == 0
    # an element at or above r, in every operand, at the first and the last position
    for v in (r, (1 << 256) - 1):
        for name, arr in (("s", st), ("k", keys), ("h", headers), ("t", texts)):
            for at in (0, arr.size // 4 - 1):
                bad = arr.copy().reshape(-1, 4)
                bad[at] = pu.limbs([v])[0]
                assert enc(**{name: p64(bad)}) == EINVAL, (name, at)
                assert dec(**{name: p64(bad)}) == EINVAL, (name, at)
        for at in (0, 4):
            bad = tags.copy()
            bad[at] = pu.limbs([v])[0]
            assert dec(g=p64(bad)) == EINVAL
    assert enc() == 0 and dec() == 0  # nothing sticks
    # in place: the output text is exactly the input text
    buf = texts.copy()
    assert enc(t=p64(buf), o=p64(buf)) == 0 and buf.tobytes() == ct.tobytes()
    assert dec(t=p64(buf), o=p64(buf)) == 0 and buf.tobytes() == texts.tobytes()
    # the Python wrappers refuse what the library refuses
    with pytest.raises(BackendError) as e:
        zb.poseidon_duplex_encrypt_host(curve.cid, st, keys, headers, np.zeros((5, 0, 3, 4), np.uint64))
    assert e.value.code == EINVAL
    with pytest.raises(ValueError):
        zb.poseidon_duplex_encrypt_host(curve.cid, st[:3], keys, headers, texts)
