"""The Poseidon duplex cipher on the device (csrc/zl_poseidon_dev.hip: k_pos_duplex) against the Python model of tests/poseidon_duplex_util.py, both curves,
widths 3..6, at the smallest shapes that reach every branch: wave and block edges, the shapes A..E, several chunks, device pointers in place and out of place,
the host paths, decryption verdicts, non-canonical input, a forked lane, a foreign stream.  Every batch carries the BOUND cases -- key, header, plaintext all
r - 1, all of them together, all zero -- which drive the lazily reduced sums of the kernel to their largest values: where a weak reduction or a bias is
missing they give a wrong word, not a fault."""
import json
import os

import numpy as np
import pytest

import poseidon_arity_util as pa
import poseidon_duplex_util as du
import poseidon_util as pu
from oracle_lib import po
from openzl_amd import backend as zb

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FX = json.load(open(os.path.join(HERE, "golden", "ref_poseidon_fixtures.json")))
CURVES = pytest.mark.parametrize("curve", pa.CURVES, ids=lambda c: c.name)
WIDTHS = pytest.mark.parametrize("width", pa.WIDTHS)
EINVAL = -1
HUGE = str(1 << 30)
N_RANDOM = 65
N_BOUND = 5


@pytest.fixture(autouse=True)
def device_path(monkeypatch):
    """every host-pointer call of this file runs on the device unless a test says otherwise"""
    monkeypatch.setenv("ZL_TUNE_POSEIDON_DEV_MIN", "0")


_REF = {}


def ref(curve, width, name):
    """(initial state, items, their encryptions (ciphertext blocks, tag)) of a shape: the five bound cases, then 65 random items; computed once per
    (curve, width, shape) and shared, never changed"""
    key = (curve.name, width, name)
    if key not in _REF:
        shape = du.shapes(width)[name]
        st = pu.random_elems(curve, width, 500 + width)
        items = du.bound_items(curve, width, shape) + du.random_items(curve, width, shape, N_RANDOM, 600 + 10 * width + ord(name))
        _REF[key] = (st, items, [du.encrypt(curve, st, *it) for it in items])
    return _REF[key]


def selection(count):
    """indices of a batch of `count` items: the bound cases first, the random ones in turn, and a bound case (all r - 1 together) in the LAST lane again"""
    sel = (list(range(N_BOUND)) + [N_BOUND + i % N_RANDOM for i in range(count)])[:count]
    if count > N_BOUND:
        sel[-1] = 3
    return sel


def batch(curve, width, name, count):
    """(state words, keys, headers, texts, expected ciphertext words, expected tag words) of a batch"""
    st, items, exp = ref(curve, width, name)
    sel = selection(count)
    keys, headers, texts = du.pack([items[i] for i in sel], width, du.shapes(width)[name])
    return pu.limbs(st), keys, headers, texts, du.text_words([exp[i][0] for i in sel], width), pu.limbs([exp[i][1] for i in sel])


def below_r(curve, *arrays):
    return all(v < curve.fr.p for a in arrays for v in pu.ints(a))


def dev(a: np.ndarray):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    return t


def host(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def encrypt_dev(backend, curve, st, keys, headers, texts, in_place):
    count, n, rate, _ = texts.shape
    d_k, d_h, d_t, d_g = dev(keys), dev(headers), dev(texts), dev(np.zeros((count, 4), dtype=np.uint64))
    d_o = d_t if in_place else dev(np.zeros_like(texts))
    backend.poseidon_duplex_encrypt_dev(curve.cid, rate + 1, st, d_k.data_ptr(), keys.shape[1], d_h.data_ptr(), headers.shape[1], d_t.data_ptr(), n, count,
                                        d_o.data_ptr(), d_g.data_ptr())
    if not in_place:
        assert host(d_t).tobytes() == texts.tobytes()  # the input is left alone
    return host(d_o).reshape(texts.shape), host(d_g).reshape(count, 4)


def decrypt_dev(backend, curve, st, keys, headers, cts, tags, in_place):
    count, n, rate, _ = cts.shape
    d_k, d_h, d_t, d_g = dev(keys), dev(headers), dev(cts), dev(tags)
    d_o = d_t if in_place else dev(np.zeros_like(cts))
    ok = backend.poseidon_duplex_decrypt_dev(curve.cid, rate + 1, st, d_k.data_ptr(), keys.shape[1], d_h.data_ptr(), headers.shape[1], d_t.data_ptr(),
                                             d_g.data_ptr(), n, count, d_o.data_ptr())
    assert host(d_g).tobytes() == tags.tobytes()
    return host(d_o).reshape(cts.shape), ok


# ---- wave and block edges, every shape, with the bound cases ------------------------------------------------------------------------------------------
@CURVES
@WIDTHS
def test_encrypt_and_decrypt_at_wave_and_block_edges(backend, curve, width):
    r = curve.fr.p
    _, items, _ = ref(curve, width, "C")
    k, h, n = du.shapes(width)["C"]
    assert items[3] == ([r - 1] * k, [r - 1] * h, [[r - 1] * (width - 1)] * n) and items[4] == ([0] * k, [0] * h, [[0] * (width - 1)] * n)
    for name, counts in [("C", (1, 63, 64, 65, 257))] + [(s, (65,)) for s in sorted(du.shapes(width)) if s != "C"]:
        for count in counts:
            st, keys, headers, texts, exp_ct, exp_tag = batch(curve, width, name, count)
            ct, tags = backend.poseidon_duplex_encrypt(curve.cid, st, keys, headers, texts)
            assert ct.shape == texts.shape and tags.shape == (count, 4)
            assert ct.tobytes() == exp_ct.tobytes() and tags.tobytes() == exp_tag.tobytes(), (name, count)
            back, ok = backend.poseidon_duplex_decrypt(curve.cid, st, keys, headers, ct, tags)
            assert ok.shape == (count,) and ok.all() and back.tobytes() == texts.tobytes(), (name, count)
            assert below_r(curve, ct, tags, back)
    e = np.zeros((0, 2, width - 1, 4), dtype=np.uint64)
    ct, tags = backend.poseidon_duplex_encrypt(curve.cid, None, np.zeros((0, 1, 4), np.uint64), np.zeros((0, 0, 4), np.uint64), e)
    assert ct.shape == e.shape and tags.shape == (0, 4)


@CURVES
@WIDTHS
def test_initial_state_all_r_minus_1(backend, curve, width):
    r = curve.fr.p
    _, items, _ = ref(curve, width, "C")
    items = items[:N_BOUND + 3]
    st = [r - 1] * width
    exp = [du.encrypt(curve, st, *it) for it in items]
    keys, headers, texts = du.pack(items, width, du.shapes(width)["C"])
    ct, tags = backend.poseidon_duplex_encrypt(curve.cid, pu.limbs(st), keys, headers, texts)
    assert ct.tobytes() == du.text_words([e[0] for e in exp], width).tobytes() and pu.ints(tags) == [e[1] for e in exp]
    back, ok = backend.poseidon_duplex_decrypt(curve.cid, pu.limbs(st), keys, headers, ct, tags)
    assert ok.all() and back.tobytes() == texts.tobytes() and below_r(curve, ct, tags, back)


@CURVES
@WIDTHS
def test_three_chunks_the_last_with_one_item(backend, curve, width, monkeypatch):
    monkeypatch.setenv("ZL_TUNE_POSEIDON_CHUNK", "256")
    st, keys, headers, texts, exp_ct, exp_tag = batch(curve, width, "A", 513)
    ct, tags = backend.poseidon_duplex_encrypt(curve.cid, st, keys, headers, texts)
    assert ct.tobytes() == exp_ct.tobytes() and tags.tobytes() == exp_tag.tobytes()
    back, ok = backend.poseidon_duplex_decrypt(curve.cid, st, keys, headers, ct, tags)
    assert ok.all() and back.tobytes() == texts.tobytes()
    ct_p, tags_p = encrypt_dev(backend, curve, st, keys, headers, texts, in_place=False)
    assert ct_p.tobytes() == exp_ct.tobytes() and tags_p.tobytes() == exp_tag.tobytes()
    bad = tags.copy()
    bad[[0, 255, 256, 512], 0] ^= np.uint64(1)  # a verdict in every chunk of the device-pointer form, which stages them per chunk
    back_p, ok_p = decrypt_dev(backend, curve, st, keys, headers, ct, bad, in_place=True)
    assert back_p.tobytes() == texts.tobytes() and [i for i in range(513) if not ok_p[i]] == [0, 255, 256, 512]


@CURVES
@WIDTHS
def test_device_device_pointer_and_host_paths_agree_byte_for_byte(backend, curve, width, monkeypatch):
    st, keys, headers, texts, exp_ct, exp_tag = batch(curve, width, "C", 130)
    enc = [backend.poseidon_duplex_encrypt(curve.cid, st, keys, headers, texts)]
    enc += [encrypt_dev(backend, curve, st, keys, headers, texts, in_place) for in_place in (True, False)]
    dec = [backend.poseidon_duplex_decrypt(curve.cid, st, keys, headers, exp_ct, exp_tag)]
    dec += [decrypt_dev(backend, curve, st, keys, headers, exp_ct, exp_tag, in_place) for in_place in (True, False)]
    monkeypatch.setenv("ZL_TUNE_POSEIDON_DEV_MIN", HUGE)
    enc += [backend.poseidon_duplex_encrypt(curve.cid, st, keys, headers, texts), zb.poseidon_duplex_encrypt_host(curve.cid, st, keys, headers, texts)]
    dec += [backend.poseidon_duplex_decrypt(curve.cid, st, keys, headers, exp_ct, exp_tag),
            zb.poseidon_duplex_decrypt_host(curve.cid, st, keys, headers, exp_ct, exp_tag)]
    for ct, tags in enc:
        assert ct.tobytes() == exp_ct.tobytes() and tags.tobytes() == exp_tag.tobytes()
    for back, ok in dec:
        assert back.tobytes() == texts.tobytes() and ok.all()


# ---- decryption verdicts ------------------------------------------------------------------------------------------------------------------------------
@CURVES
@WIDTHS
def test_decrypt_verdicts_and_plaintexts_of_corrupted_items(backend, curve, width):
    """one corruption each at items 0, 63, 64, 129: the first ciphertext element + 1, the last element of the last block + 1, the tag + 1, a key element changed"""
    r, count = curve.fr.p, 130
    st_ints, items, exp = ref(curve, width, "C")
    sel = selection(count)
    st, keys, headers, texts, ct, tags = batch(curve, width, "C", count)
    keys, ct, tags = keys.copy(), ct.copy(), tags.copy()
    plus1 = lambda w: pu.limbs([(pu.ints(w)[0] + 1) % r])[0]
    ct[0, 0, 0] = plus1(ct[0, 0, 0])
    ct[63, -1, -1] = plus1(ct[63, -1, -1])
    tags[64] = plus1(tags[64])
    keys[129, 1] = plus1(keys[129, 1])
    want = texts.copy()
    for i in (0, 63, 129):  # (item 64, whose tag alone is wrong, keeps its plaintext)
        key = pu.ints(keys[i])
        blocks = [pu.ints(b) for b in ct[i]]
        plain, ok = du.decrypt(curve, st_ints, key, items[sel[i]][1], blocks, pu.ints(tags[i])[0])
        assert not ok
        want[i] = du.text_words([plain], width)[0]
    assert du.decrypt(curve, st_ints, *items[sel[64]][:2], exp[sel[64]][0], pu.ints(tags[64])[0]) == (items[sel[64]][2], False)
    mask = [i not in (0, 63, 64, 129) for i in range(count)]
    for back, ok in (backend.poseidon_duplex_decrypt(curve.cid, st, keys, headers, ct, tags), decrypt_dev(backend, curve, st, keys, headers, ct, tags, True),
                     zb.poseidon_duplex_decrypt_host(curve.cid, st, keys, headers, ct, tags)):
        assert list(ok) == mask
        assert back.tobytes() == want.tobytes() and below_r(curve, back[[0, 63, 64, 129]])
    assert want[64].tobytes() == texts[64].tobytes() and want[0].tobytes() != texts[0].tobytes()


# ---- non-canonical input ------------------------------------------------------------------------------------------------------------------------------
@CURVES
@WIDTHS
def test_non_canonical_input_is_refused(backend, curve, width):
    st, keys, headers, texts, ct, tags = batch(curve, width, "C", 65)
    at_r = pu.limbs([curve.fr.p])[0]
    for which in range(4):
        for at in (0, -1):
            ops = [keys.copy(), headers.copy(), texts.copy(), tags.copy()]
            ops[which].reshape(-1, 4)[at] = at_r
            calls = [lambda: backend.poseidon_duplex_decrypt(curve.cid, st, ops[0], ops[1], ops[2], ops[3]),
                     lambda: decrypt_dev(backend, curve, st, ops[0], ops[1], ops[2], ops[3], False)]
            if which < 3:
                calls += [lambda: backend.poseidon_duplex_encrypt(curve.cid, st, ops[0], ops[1], ops[2]),
                          lambda: encrypt_dev(backend, curve, st, ops[0], ops[1], ops[2], True)]
            for call in calls:
                with pytest.raises(zb.BackendError) as e:
                    call()
                assert e.value.code == EINVAL, (which, at)
            # the flag does not stick
            got_ct, got_tags = backend.poseidon_duplex_encrypt(curve.cid, st, keys, headers, texts)
            assert got_ct.tobytes() == ct.tobytes() and got_tags.tobytes() == tags.tobytes()
    bad_st = st.copy()
    bad_st[-1] = at_r
    with pytest.raises(zb.BackendError) as e:
        backend.poseidon_duplex_encrypt(curve.cid, bad_st, keys, headers, texts)
    assert e.value.code == EINVAL
    back, ok = decrypt_dev(backend, curve, st, keys, headers, ct, tags, True)
    assert ok.all() and back.tobytes() == texts.tobytes()


# ---- lanes and streams --------------------------------------------------------------------------------------------------------------------------------
@CURVES
def test_forked_lane_and_foreign_stream(backend, curve):
    import torch

    width = 5
    st, keys, headers, texts, exp_ct, exp_tag = batch(curve, width, "C", 65)
    lane = backend.fork()
    try:
        ct, tags = lane.poseidon_duplex_encrypt(curve.cid, st, keys, headers, texts)
        assert ct.tobytes() == exp_ct.tobytes() and tags.tobytes() == exp_tag.tobytes()
        back, ok = lane.poseidon_duplex_decrypt(curve.cid, st, keys, headers, ct, tags)
        assert ok.all() and back.tobytes() == texts.tobytes()
    finally:
        lane.close()
        backend._forks.remove(lane)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        backend.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            ct, tags = encrypt_dev(backend, curve, st, keys, headers, texts, in_place=False)
            assert ct.tobytes() == exp_ct.tobytes() and tags.tobytes() == exp_tag.tobytes()
            back, ok = backend.poseidon_duplex_decrypt(curve.cid, st, keys, headers, ct, tags)
            assert ok.all() and back.tobytes() == texts.tobytes()
        finally:
            backend.set_stream(0)


def test_anchor_to_the_reference_permutation_fixture(backend):
    """BLS12-381, width 3, [3, 1, 2], no key, no header, plaintext [0, 0]: the ciphertext is lanes 1 and 2 of the permutation of the reference's output"""
    curve = po.BLS12_381
    first = [int(v) for v in FX["permutation_width3"]["output"]]
    second = pa.permute(curve, first)
    ct, tags = backend.poseidon_duplex_encrypt(curve.cid, pu.limbs([3, 1, 2]), np.zeros((1, 0, 4), np.uint64), np.zeros((1, 0, 4), np.uint64),
                                               np.zeros((1, 1, 2, 4), np.uint64))
    assert pu.ints(ct) == second[1:] and pu.ints(tags) == [pa.permute(curve, second)[1]]
