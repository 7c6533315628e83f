"""The embedded twisted Edwards curves and the hybrid encryption on the HOST path (csrc/zl_edwards.h through zl_ed_* / zl_hybrid_* with a null ctx) against the
Python-integer model of tests/edwards_util.py, both curves: constants, the unified addition on small-order points, the windowed multiplication at the scalars
where a digit, a window or a carry can go wrong, every status code, strides, argument checks, and the hybrid cipher against the model and the duplex call."""
import ctypes as C

import numpy as np
import pytest

import edwards_util as eu
import poseidon_util as pu
from openzl_amd import backend as zb

CURVES = pytest.mark.parametrize("curve", eu.CURVES, ids=lambda c: c.name)
EINVAL = -1
ID, SHAPES, ref, hybrid_ref, hybrid_words = eu.ID, eu.SHAPES, eu.ref, eu.hybrid_ref, eu.hybrid_words


def L():
    return zb.load_library()


def p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def one_mul(curve, p, k):
    """zl_ed_scalar_mul -> (rc, point)"""
    pw, kw, out = eu.point_words([p])[0].copy(), pu.limbs([k])[0].copy(), np.zeros((2, 4), dtype=np.uint64)
    rc = L().zl_ed_scalar_mul(curve.cid, p64(pw), p64(kw), p64(out))
    return rc, eu.points_of(out)[0]


@CURVES
def test_params_equal_the_model(curve):
    q, a, d, l = eu.params(curve)
    got = zb.ed_params(curve.cid)
    assert got == {"a": a, "d": d, "order": l, "cofactor": eu.COFACTOR}
    assert eu.is_square(got["a"], q) and not eu.is_square(got["d"], q)  # complete: no exceptional case
    assert L().zl_ed_params(curve.cid, None, None, None, None) == 0  # a NULL output is skipped
    assert L().zl_ed_params(7, None, None, None, None) == EINVAL


@CURVES
def test_eight_p_lies_in_the_subgroup(curve):
    """l (8 P) = (0, 1): the library's own subgroup test accepts 8 P, and (l - 1)(8 P) + 8 P is the identity"""
    l = eu.params(curve)[3]
    pts = eu.subgroup_points(curve, 4, 21)
    out, st = zb.ed_scalar_mul_host(curve.cid, eu.point_words(pts), pu.limbs([l - 1] * 4), check_subgroup=True)
    assert st.tolist() == [0] * 4
    for p, r in zip(pts, out):
        assert eu.points_of(zb.ed_add_host(curve.cid, r, eu.point_words([p])[0]))[0] == ID


@CURVES
def test_add_against_the_model(curve):
    pts = ref(curve)[0]
    for p in pts:
        for r in pts:
            assert eu.points_of(zb.ed_add_host(curve.cid, eu.point_words([p])[0], eu.point_words([r])[0]))[0] == eu.add(curve, p, r)


@CURVES
def test_scalar_mul_against_the_model(curve):
    pts, ks, pairs, want = ref(curve)
    out, st = zb.ed_scalar_mul_host(curve.cid, eu.point_words([p for p, _ in pairs]), pu.limbs([k for _, k in pairs]))
    assert not st.any()
    assert eu.points_of(out) == want
    for i in range(0, len(pairs), 17):  # the one-item entry point on a sample
        assert one_mul(curve, *pairs[i]) == (0, want[i])
    assert all(want[i] == ID for i in range(len(ks)))  # k (0, 1) = (0, 1)


@CURVES
def test_diffie_hellman_agrees(curve):
    g = eu.subgroup_points(curve, 1, 31)[0]
    a, b = eu.random_scalars(curve, 2, 32)
    ag, _ = zb.ed_scalar_mul_host(curve.cid, eu.point_words([g])[0], pu.limbs([a, b]))
    ab, st = zb.ed_scalar_mul_host(curve.cid, ag[::-1].copy(), pu.limbs([a, b]))
    assert not st.any() and ab[0].tobytes() == ab[1].tobytes() and eu.points_of(ab)[0] == eu.mul(curve, a * b, g)


def bad_batch(curve):
    """nine items, the bad ones with good neighbours: (points, scalars, check flag needed, expected status)"""
    q, a, d, l = eu.params(curve)
    good = eu.subgroup_points(curve, 9, 41)
    ks = eu.random_scalars(curve, 9, 42)
    pts = list(good)
    pts[1] = (q, good[1][1])                                     # x = q: 1
    pts[2] = (good[2][0], (1 << 256) - 1)                        # y = 2^256 - 1: 1
    pts[4] = (good[4][0], (good[4][1] + 1) % q)                  # off the curve: 2
    pts[6] = eu.add(curve, good[6], eu.small_order_points(curve)[2])  # outside the subgroup: 3 with the flag
    ks[7] = l                                                    # 4
    ks[8] = (1 << 256) - 1                                       # 4
    return pts, ks, [0, 1, 1, 0, 2, 0, 3, 4, 4]


@CURVES
def test_every_status_code_and_the_neighbours(curve):
    pts, ks, want = bad_batch(curve)
    assert not eu.on_curve(curve, pts[4])
    for check in (False, True):
        exp = [s if (s != 3 or check) else 0 for s in want]
        out, st = zb.ed_scalar_mul_host(curve.cid, eu.point_words(pts), pu.limbs(ks), check_subgroup=check)
        assert st.tolist() == exp
        for i, (r, s) in enumerate(zip(eu.points_of(out), exp)):
            assert r == (ID if s else eu.mul(curve, ks[i], pts[i])), i
        # status == NULL: the whole call is refused
        o = np.zeros((9, 2, 4), dtype=np.uint64)
        assert L().zl_ed_scalar_mul_batch(None, curve.cid, p64(eu.point_words(pts)), 1, p64(pu.limbs(ks)), 1, 9, 1 if check else 0, p64(o), None) == EINVAL
    ok = [i for i, s in enumerate(want) if s == 0]
    o = np.zeros((len(ok), 2, 4), dtype=np.uint64)
    assert L().zl_ed_scalar_mul_batch(None, curve.cid, p64(eu.point_words([pts[i] for i in ok])), 1, p64(pu.limbs([ks[i] for i in ok])), 1, len(ok), 1, p64(o), None) == 0
    # the one-item forms refuse the same operands
    assert one_mul(curve, pts[1], 1)[0] == EINVAL and one_mul(curve, pts[4], 1)[0] == EINVAL and one_mul(curve, pts[0], ks[7])[0] == EINVAL
    with pytest.raises(zb.BackendError):
        zb.ed_add_host(curve.cid, eu.point_words([pts[4]])[0], eu.point_words([pts[0]])[0])


@CURVES
def test_strides_agree_with_the_replicated_form(curve):
    pts = eu.random_points(curve, 5, 51)
    ks = eu.random_scalars(curve, 5, 52)
    pw, kw = eu.point_words(pts), pu.limbs(ks)
    full, _ = zb.ed_scalar_mul_host(curve.cid, pw, kw)
    shared_p, st = zb.ed_scalar_mul_host(curve.cid, pw[2], kw)
    assert not st.any() and shared_p.tobytes() == zb.ed_scalar_mul_host(curve.cid, np.repeat(pw[2:3], 5, axis=0), kw)[0].tobytes()
    shared_k, st = zb.ed_scalar_mul_host(curve.cid, pw, kw[3])
    assert not st.any() and shared_k.tobytes() == zb.ed_scalar_mul_host(curve.cid, pw, np.repeat(kw[3:4], 5, axis=0))[0].tobytes()
    assert shared_p[2].tobytes() == full[2].tobytes() and shared_k[3].tobytes() == full[3].tobytes()
    both, _ = zb.ed_scalar_mul_host(curve.cid, pw[1], kw[1])
    assert both.shape == (1, 2, 4) and both[0].tobytes() == full[1].tobytes()
    # only a bare scalar (4,) or point (2, 4) broadcasts: a (1, 4) / (1, 2, 4) array is a batch of one and does not match five items
    one, _ = zb.ed_scalar_mul_host(curve.cid, pw[1:2], kw[1:2])
    assert one.tobytes() == both.tobytes()
    with pytest.raises(ValueError):
        zb.ed_scalar_mul_host(curve.cid, pw, kw[3:4])
    with pytest.raises(ValueError):
        zb.ed_scalar_mul_host(curve.cid, pw[2:3], kw)


def test_scalar_mul_argument_checks():
    curve = eu.CURVES[0]
    pw, kw = eu.point_words(eu.random_points(curve, 2, 61)), pu.limbs([3, 4])
    out, st = np.zeros((2, 2, 4), dtype=np.uint64), np.zeros(2, dtype=np.uint8)
    sp = st.ctypes.data_as(C.POINTER(C.c_uint8))
    call = L().zl_ed_scalar_mul_batch
    assert call(None, curve.cid, p64(pw), 1, p64(kw), 1, 2, 0, p64(out), sp) == 0
    assert call(None, curve.cid, None, 1, None, 1, 0, 0, None, None) == 0          # count == 0 writes nothing
    assert call(None, 0, p64(pw), 1, p64(kw), 1, 2, 0, p64(out), sp) == EINVAL     # unknown curve
    assert call(None, curve.cid, p64(pw), 2, p64(kw), 1, 2, 0, p64(out), sp) == EINVAL
    assert call(None, curve.cid, p64(pw), 1, p64(kw), 2, 2, 0, p64(out), sp) == EINVAL
    assert call(None, curve.cid, p64(pw), 1, p64(kw), 1, 2, 2, p64(out), sp) == EINVAL  # unknown flag
    assert call(None, curve.cid, None, 1, p64(kw), 1, 2, 0, p64(out), sp) == EINVAL
    assert call(None, curve.cid, p64(pw), 1, None, 1, 2, 0, p64(out), sp) == EINVAL
    assert call(None, curve.cid, p64(pw), 1, p64(kw), 1, 2, 0, None, sp) == EINVAL
    assert L().zl_ed_scalar_mul_batch_dev(None, curve.cid, None, 1, None, 1, 0, 0, None, None) == EINVAL  # the device form has no host path
    assert L().zl_ed_add(curve.cid, None, p64(pw), p64(out)) == EINVAL and L().zl_ed_scalar_mul(curve.cid, p64(pw), None, p64(out)) == EINVAL


# ---- hybrid encryption ---------------------------------------------------------------------------------------------------------------------------------------
@CURVES
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_hybrid_host_against_the_model(curve, shape):
    w = hybrid_words(curve, shape)
    st, g, esks, sks, pks, headers, texts, enc = hybrid_ref(curve, shape)
    epk, ct, tag, status = zb.hybrid_encrypt_host(curve.cid, w["st"], w["g"], w["esk"], w["pk"], w["h"], w["t"])
    assert not status.any()
    assert epk.tobytes() == w["epk"].tobytes() and ct.tobytes() == w["ct"].tobytes() and tag.tobytes() == w["tag"].tobytes()
    # the same ciphertext as the duplex call under the model's shared secret
    secrets = eu.point_words([eu.mul(curve, e, p) for e, p in zip(esks, pks)])
    ct2, tag2 = zb.poseidon_duplex_encrypt_host(curve.cid, w["st"], secrets, w["h"], w["t"])
    assert ct2.tobytes() == ct.tobytes() and tag2.tobytes() == tag.tobytes()
    # decrypt(encrypt) with every recipient's own key
    pt, ok, status = zb.hybrid_decrypt_host(curve.cid, w["st"], w["sk"], epk, w["h"], ct, tag)
    assert ok.all() and not status.any() and pt.tobytes() == w["t"].tobytes()
    assert eu.hybrid_decrypt(curve, st, sks[0], enc[0][0], headers[0], enc[0][1], enc[0][2]) == (texts[0], True)
    # a wrong secret key, a flipped tag, a flipped ciphertext element
    wrong = w["sk"].copy()
    wrong[1] = pu.limbs([(sks[1] + 1) % eu.params(curve)[3]])[0]
    bad_tag = tag.copy()
    bad_tag[2, 0] ^= np.uint64(1)
    bad_ct = ct.copy()
    bad_ct[3, 0, 0, 0] ^= np.uint64(1)
    for sk_, ct_, tag_, item in ((wrong, ct, tag, 1), (w["sk"], ct, bad_tag, 2), (w["sk"], bad_ct, tag, 3)):
        pt, ok, status = zb.hybrid_decrypt_host(curve.cid, w["st"], sk_, epk, w["h"], ct_, tag_)
        assert ok.tolist() == [i != item for i in range(len(esks))] and not status.any()
    # one key for all items (the scan): only its own message opens
    pt, ok, status = zb.hybrid_decrypt_host(curve.cid, w["st"], w["sk"][4], epk, w["h"], ct, tag)
    assert ok.tolist() == [i == 4 for i in range(len(esks))] and pt[4].tobytes() == w["t"][4].tobytes()
    # one public key for all items
    e1, c1, t1, _ = zb.hybrid_encrypt_host(curve.cid, w["st"], w["g"], w["esk"], w["pk"][2], w["h"], w["t"])
    e2, c2, t2, _ = zb.hybrid_encrypt_host(curve.cid, w["st"], w["g"], w["esk"], np.repeat(w["pk"][2:3], len(esks), axis=0), w["h"], w["t"])
    assert (e1.tobytes(), c1.tobytes(), t1.tobytes()) == (e2.tobytes(), c2.tobytes(), t2.tobytes()) and c1[2].tobytes() == ct[2].tobytes()


@CURVES
def test_hybrid_bad_points_never_fail_a_decryption(curve):
    shape = SHAPES[0]
    w = hybrid_words(curve, shape)
    q = curve.fr.p
    epk, ct, tag, _ = zb.hybrid_encrypt_host(curve.cid, w["st"], w["g"], w["esk"], w["pk"], w["h"], w["t"])
    bad = epk.copy()
    bad[1, 0] = pu.limbs([q])[0]                                   # a coordinate >= q
    bad[3, 1] = pu.limbs([(pu.ints(epk[3, 1])[0] + 1) % q])[0]     # off the curve
    pt, ok, status = zb.hybrid_decrypt_host(curve.cid, w["st"], w["sk"], bad, w["h"], ct, tag)
    assert status.tolist() == [0, 1, 0, 2, 0, 0] and ok.tolist() == [True, False, True, False, True, True]
    assert pt[0].tobytes() == w["t"][0].tobytes() and pt[2].tobytes() == w["t"][2].tobytes()
    # encryption reports a bad recipient key per item and leaves epk = (0, 1) there
    pk = w["pk"].copy()
    pk[2, 1] = pu.limbs([(pu.ints(pk[2, 1])[0] + 1) % q])[0]
    e, c, t, status = zb.hybrid_encrypt_host(curve.cid, w["st"], w["g"], w["esk"], pk, w["h"], w["t"])
    assert status.tolist() == [0, 0, 2, 0, 0, 0] and eu.points_of(e[2])[0] == ID
    assert e[1].tobytes() == epk[1].tobytes() and c[3].tobytes() == ct[3].tobytes()


def test_hybrid_argument_checks():
    curve = eu.CURVES[1]
    w = hybrid_words(curve, SHAPES[0])
    n = w["esk"].shape[0]
    epk, ct, tag, st = np.zeros((n, 2, 4), dtype=np.uint64), np.zeros_like(w["t"]), np.zeros((n, 4), dtype=np.uint64), np.zeros(n, dtype=np.uint8)
    ok = np.zeros(n, dtype=np.uint8)
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))

    def enc(cid=curve.cid, width=3, g=w["g"], esk=w["esk"], pk=w["pk"], ps=1, hlen=0, blocks=1, count=n, flags=0, e=epk, c=ct, t=tag, text=w["t"]):
        f = lambda a: None if a is None else p64(a)
        return L().zl_hybrid_encrypt_batch(None, cid, width, p64(w["st"]), f(g), f(esk), f(pk), ps, None, hlen, f(text), blocks, count, flags, f(e), f(c), f(t), u8(st))

    def dec(cid=curve.cid, width=3, sk=w["sk"], ks=1, e=w["epk"], hlen=0, blocks=1, count=n, flags=0, c=w["ct"], t=w["tag"], out=ct, okp=ok):
        f = lambda a: None if a is None else p64(a)
        return L().zl_hybrid_decrypt_batch(None, cid, width, p64(w["st"]), f(sk), ks, f(e), None, hlen, f(c), f(t), blocks, count, flags, f(out),
                                           None if okp is None else u8(okp), u8(st))

    assert enc() == 0 and dec() == 0 and ok.all()
    assert enc(count=0, g=None, esk=None, pk=None, e=None, c=None, t=None, text=None) == 0
    assert dec(count=0, sk=None, e=None, c=None, t=None, out=None, okp=None) == 0
    for kw in (dict(cid=9), dict(width=2), dict(width=7), dict(ps=2), dict(hlen=65), dict(blocks=0), dict(blocks=1025), dict(flags=2), dict(g=None), dict(esk=None),
               dict(pk=None), dict(e=None), dict(c=None), dict(t=None), dict(text=None), dict(hlen=1)):
        assert enc(**kw) == EINVAL, kw
    for kw in (dict(cid=9), dict(width=2), dict(ks=2), dict(hlen=65), dict(blocks=0), dict(flags=4), dict(sk=None), dict(e=None), dict(c=None), dict(t=None),
               dict(out=None), dict(okp=None), dict(hlen=1)):
        assert dec(**kw) == EINVAL, kw
    # a text element >= r stays the duplex call's ZL_EINVAL
    big = w["t"].copy()
    big[0, 0, 0] = pu.limbs([curve.fr.p])[0]
    assert enc(text=big) == EINVAL and dec(c=big) == EINVAL
    assert L().zl_hybrid_encrypt_batch_dev(None, curve.cid, 3, None, p64(w["g"]), None, None, 1, None, 0, None, 1, 0, 0, None, None, None, None) == EINVAL
    assert L().zl_hybrid_decrypt_batch_dev(None, curve.cid, 3, None, None, 1, None, None, 0, None, None, 1, 0, 0, None, None, None) == EINVAL
