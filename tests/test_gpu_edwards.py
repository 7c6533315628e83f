"""Embedded-curve scalar multiplication and hybrid encryption on the device (csrc/zl_edwards_dev.hip: k_ed_mul, k_ed_mul_fixed) against the host mirror byte for
byte and against the Python model of tests/edwards_util.py on its sample, both curves, at the smallest shapes that reach every path: wave and block edges,
several chunks, per-item and shared operands on both sides of the fixed-base bound, the subgroup flag, refused items at lane and chunk edges, device pointers,
and the hybrid cipher with the scan of one key over a batch."""
import numpy as np
import pytest

import edwards_util as eu
import poseidon_util as pu
from openzl_amd import backend as zb

pytestmark = pytest.mark.gpu

ID, SHAPES, ref, hybrid_ref, hybrid_words = eu.ID, eu.SHAPES, eu.ref, eu.hybrid_ref, eu.hybrid_words
CURVES = pytest.mark.parametrize("curve", eu.CURVES, ids=lambda c: c.name)
COUNTS = [1, 63, 64, 65, 130, 257]
HUGE = str(1 << 30)


@pytest.fixture(autouse=True)
def device_path(monkeypatch):
    """every host-pointer call of this file runs on the device unless a test says otherwise"""
    monkeypatch.setenv("ZL_TUNE_ED_DEV_MIN", "0")
    monkeypatch.setenv("ZL_TUNE_POSEIDON_DEV_MIN", "0")


def dev(a: np.ndarray):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    return t


def host64(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def batch(curve, count):
    """`count` (point, scalar) pairs cycling through the host tests' reference set -- the identity, small-order points, mixed points, the edge scalars -- and
    the model products of the same pairs"""
    pts, ks, pairs, want = ref(curve)
    sel = [(7 * i) % len(pairs) for i in range(count)]
    return eu.point_words([pairs[i][0] for i in sel]), pu.limbs([pairs[i][1] for i in sel]), [want[i] for i in sel]


@CURVES
@pytest.mark.parametrize("count", COUNTS)
def test_per_item_operands(backend, curve, count):
    pw, kw, want = batch(curve, count)
    out, st = backend.ed_scalar_mul(curve.cid, pw, kw)
    h_out, h_st = zb.ed_scalar_mul_host(curve.cid, pw, kw)
    assert not st.any() and out.tobytes() == h_out.tobytes()
    assert eu.points_of(out) == want


@CURVES
def test_several_chunks(backend, curve, monkeypatch):
    monkeypatch.setenv("ZL_TUNE_ED_CHUNK", "128")  # 257 items: 128 + 128 + 1
    pw, kw, want = batch(curve, 257)
    out, st = backend.ed_scalar_mul(curve.cid, pw, kw)
    assert not st.any() and eu.points_of(out) == want
    out, st = backend.ed_scalar_mul(curve.cid, pw[5], kw)  # the fixed-base kernel, chunked
    assert not st.any() and out.tobytes() == zb.ed_scalar_mul_host(curve.cid, pw[5], kw)[0].tobytes()


@CURVES
def test_shared_point_on_both_sides_of_the_fixed_base_bound(backend, curve, monkeypatch):
    pw, kw, _ = batch(curve, 130)
    p = eu.point_words(eu.random_points(curve, 1, 81))[0]
    h_out, _ = zb.ed_scalar_mul_host(curve.cid, p, kw)
    model = [eu.mul(curve, k, eu.points_of(p)[0]) for k in pu.ints(kw[:24])]
    for count in (40, 130):  # below the bound: k_ed_mul with every lane on the same point; from it: k_ed_mul_fixed
        out, st = backend.ed_scalar_mul(curve.cid, p, kw[:count])
        assert not st.any() and out.tobytes() == h_out[:count].tobytes()
        assert eu.points_of(out[:24]) == model
    monkeypatch.setenv("ZL_TUNE_ED_FIXED_MIN", HUGE)  # ... and the variable-base kernel at the larger count
    out, st = backend.ed_scalar_mul(curve.cid, p, kw)
    assert not st.any() and out.tobytes() == h_out.tobytes()
    # a shared point outside the subgroup, with the flag, is refused for every item by either kernel
    monkeypatch.delenv("ZL_TUNE_ED_FIXED_MIN")
    mixed = eu.point_words([eu.add(curve, eu.mul(curve, eu.COFACTOR, eu.points_of(p)[0]), eu.small_order_points(curve)[1])])[0]
    for count in (40, 130):
        out, st = backend.ed_scalar_mul(curve.cid, mixed, kw[:count], check_subgroup=True)
        assert st.tolist() == [3] * count and eu.points_of(out) == [ID] * count


@CURVES
def test_shared_scalar(backend, curve):
    pw, kw, _ = batch(curve, 130)
    k = pu.limbs(eu.random_scalars(curve, 1, 82))[0]
    out, st = backend.ed_scalar_mul(curve.cid, pw, k)
    assert not st.any() and out.tobytes() == zb.ed_scalar_mul_host(curve.cid, pw, k)[0].tobytes()
    assert eu.points_of(out[:24]) == [eu.mul(curve, pu.ints(k)[0], p) for p in eu.points_of(pw[:24])]


@CURVES
def test_subgroup_flag_on_a_mixed_batch(backend, curve):
    sub = eu.subgroup_points(curve, 3, 83)
    small = eu.small_order_points(curve)
    pts = [eu.add(curve, sub[i % 3], small[i % 3]) if i % 4 == 1 else sub[i % 3] for i in range(70)]
    kw = pu.limbs(eu.random_scalars(curve, 70, 84))
    out, st = backend.ed_scalar_mul(curve.cid, eu.point_words(pts), kw, check_subgroup=True)
    h_out, h_st = zb.ed_scalar_mul_host(curve.cid, eu.point_words(pts), kw, check_subgroup=True)
    assert st.tolist() == [3 if i % 4 == 1 else 0 for i in range(70)] == h_st.tolist() and out.tobytes() == h_out.tobytes()
    out, st = backend.ed_scalar_mul(curve.cid, eu.point_words(pts), kw)  # without the flag the same points multiply
    assert not st.any() and eu.points_of(out[:8]) == [eu.mul(curve, k, p) for k, p in zip(pu.ints(kw[:8]), pts[:8])]


@CURVES
def test_refused_items_at_lane_and_chunk_edges(backend, curve, monkeypatch):
    monkeypatch.setenv("ZL_TUNE_ED_CHUNK", "128")
    q, a, d, l = eu.params(curve)
    pw, kw, want = batch(curve, 257)
    pw, kw = pw.copy(), kw.copy()
    exp = {0: 1, 31: 2, 63: 4, 127: 2, 128: 1, 256: 4}
    for i, code in exp.items():
        if code == 1:
            pw[i, 0] = pu.limbs([q])[0]
        elif code == 2:
            good = eu.random_points(curve, 1, 90 + i)[0]
            pw[i] = eu.point_words([(good[0], (good[1] + 1) % q)])[0]
        else:
            kw[i] = pu.limbs([l])[0]
    out, st = backend.ed_scalar_mul(curve.cid, pw, kw)
    h_out, h_st = zb.ed_scalar_mul_host(curve.cid, pw, kw)
    assert st.tolist() == [exp.get(i, 0) for i in range(257)] == h_st.tolist() and out.tobytes() == h_out.tobytes()
    got = eu.points_of(out)
    assert all(got[i] == (ID if i in exp else want[i]) for i in range(257))  # the neighbours are untouched
    # status == NULL: the flag word refuses the call
    o = np.zeros((257, 2, 4), dtype=np.uint64)
    assert backend.L.zl_ed_scalar_mul_batch(backend._ctx, curve.cid, zb._p64(pw), 1, zb._p64(kw), 1, 257, 0, zb._p64(o), None) == -1
    assert backend.L.zl_ed_scalar_mul_batch(backend._ctx, curve.cid, zb._p64(pw[1:31]), 1, zb._p64(kw[1:31]), 1, 30, 0, zb._p64(o), None) == 0
    assert o[:30].tobytes() == h_out[1:31].tobytes()


@CURVES
def test_device_pointers(backend, curve):
    pw, kw, want = batch(curve, 130)
    kw = kw.copy()
    kw[64] = pu.limbs([eu.params(curve)[3]])[0]
    h_out, h_st = zb.ed_scalar_mul_host(curve.cid, pw, kw)
    d_p, d_k, d_o, d_s = dev(pw), dev(kw), dev(np.zeros_like(pw)), dev(np.zeros(130, dtype=np.uint8))
    backend.ed_scalar_mul_dev(curve.cid, d_p.data_ptr(), 1, d_k.data_ptr(), 1, 130, d_o.data_ptr(), d_s.data_ptr())
    assert host64(d_o).tobytes() == h_out.tobytes() and d_s.cpu().numpy().tolist() == h_st.tolist() and h_st[64] == 4
    assert host64(d_p).tobytes() == pw.tobytes() and host64(d_k).tobytes() == kw.tobytes()  # the inputs are left alone
    # strides 0 on device operands: the fixed-base kernel (the point is fetched once for its table), then the shared scalar
    backend.ed_scalar_mul_dev(curve.cid, d_p.data_ptr() + 64 * 3, 0, d_k.data_ptr(), 1, 130, d_o.data_ptr(), d_s.data_ptr())
    assert host64(d_o).tobytes() == zb.ed_scalar_mul_host(curve.cid, pw[3], kw)[0].tobytes()
    backend.ed_scalar_mul_dev(curve.cid, d_p.data_ptr(), 1, d_k.data_ptr() + 32 * 2, 0, 130, d_o.data_ptr(), d_s.data_ptr())
    assert host64(d_o).tobytes() == zb.ed_scalar_mul_host(curve.cid, pw, kw[2])[0].tobytes() and not d_s.cpu().numpy().any()
    with pytest.raises(zb.BackendError):  # no status array: the refused item fails the call
        backend.ed_scalar_mul_dev(curve.cid, d_p.data_ptr(), 1, d_k.data_ptr(), 1, 130, d_o.data_ptr(), 0)


# ---- hybrid encryption ---------------------------------------------------------------------------------------------------------------------------------------
_SCAN = {}


def scan_batch(curve, shape, count=130, ours=(0, 1, 64, 129)):
    """`count` messages of which `ours` are addressed to key 0 and the rest to other keys, encrypted by the HOST mirror (pinned to the model by
    tests/test_edwards_host.py); computed once per (curve, shape)"""
    key = (curve.name, shape)
    if key not in _SCAN:
        width, h, n = shape
        rate = width - 1
        w = hybrid_words(curve, shape)
        st, g, esks, sks, pks, headers, texts, enc = hybrid_ref(curve, shape)
        who = [0 if i in ours else 1 + i % (len(sks) - 1) for i in range(count)]
        esk = pu.limbs(eu.random_scalars(curve, count, 101))
        pk = w["pk"][who]
        vals = pu.random_elems(curve, count * (h + n * rate), 102)
        hd = pu.limbs(vals[:count * h]).reshape(count, h, 4)
        tx = pu.limbs(vals[count * h:]).reshape(count, n, rate, 4)
        epk, ct, tag, status = zb.hybrid_encrypt_host(curve.cid, w["st"], w["g"], esk, pk, hd, tx)
        assert not status.any()
        _SCAN[key] = dict(st=w["st"], g=w["g"], esk=esk, pk=pk, sk=w["sk"][who], sk0=w["sk"][0], h=hd, t=tx, epk=epk, ct=ct, tag=tag, ours=list(ours))
    return _SCAN[key]


@CURVES
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_hybrid_on_the_device(backend, curve, shape):
    w = hybrid_words(curve, shape)
    n = w["esk"].shape[0]
    # the model's sample, below the fixed-base bound ...
    epk, ct, tag, status = backend.hybrid_encrypt(curve.cid, w["st"], w["g"], w["esk"], w["pk"], w["h"], w["t"])
    assert not status.any() and epk.tobytes() == w["epk"].tobytes() and ct.tobytes() == w["ct"].tobytes() and tag.tobytes() == w["tag"].tobytes()
    pt, ok, status = backend.hybrid_decrypt(curve.cid, w["st"], w["sk"], epk, w["h"], ct, tag)
    assert ok.all() and not status.any() and pt.tobytes() == w["t"].tobytes() and n < 64
    # ... and 130 items against the host mirror: the ephemeral keys through the fixed-base kernel
    s = scan_batch(curve, shape)
    epk, ct, tag, status = backend.hybrid_encrypt(curve.cid, s["st"], s["g"], s["esk"], s["pk"], s["h"], s["t"])
    assert not status.any() and epk.tobytes() == s["epk"].tobytes() and ct.tobytes() == s["ct"].tobytes() and tag.tobytes() == s["tag"].tobytes()
    pt, ok, status = backend.hybrid_decrypt(curve.cid, s["st"], s["sk"], epk, s["h"], ct, tag)
    assert ok.all() and not status.any() and pt.tobytes() == s["t"].tobytes()


@CURVES
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_scan_with_one_key(backend, curve, shape, monkeypatch):
    s = scan_batch(curve, shape)
    h_pt, h_ok, h_st = zb.hybrid_decrypt_host(curve.cid, s["st"], s["sk0"], s["epk"], s["h"], s["ct"], s["tag"])
    for chunk in ("65536", "64"):  # one chunk, then three
        monkeypatch.setenv("ZL_TUNE_ED_CHUNK", chunk)
        pt, ok, status = backend.hybrid_decrypt(curve.cid, s["st"], s["sk0"], s["epk"], s["h"], s["ct"], s["tag"])
        assert np.flatnonzero(ok).tolist() == s["ours"] and not status.any()
        assert pt[s["ours"]].tobytes() == s["t"][s["ours"]].tobytes()
        assert pt.tobytes() == h_pt.tobytes() and ok.tolist() == h_ok.tolist()


@CURVES
def test_hybrid_refused_points_on_the_device(backend, curve):
    s = scan_batch(curve, SHAPES[0])
    q = curve.fr.p
    bad = s["epk"].copy()
    bad[0, 0] = pu.limbs([q])[0]
    bad[64, 1] = pu.limbs([(pu.ints(bad[64, 1])[0] + 1) % q])[0]
    pt, ok, status = backend.hybrid_decrypt(curve.cid, s["st"], s["sk0"], bad, s["h"], s["ct"], s["tag"])
    h_pt, h_ok, h_st = zb.hybrid_decrypt_host(curve.cid, s["st"], s["sk0"], bad, s["h"], s["ct"], s["tag"])
    assert np.flatnonzero(status).tolist() == [0, 64] and status[0] == 1 and status[64] == 2 and np.flatnonzero(ok).tolist() == [1, 129]
    assert status.tolist() == h_st.tolist() and ok.tolist() == h_ok.tolist() and pt.tobytes() == h_pt.tobytes()
    pk = s["pk"].copy()
    pk[63, 1] = pu.limbs([(pu.ints(pk[63, 1])[0] + 1) % q])[0]
    got = backend.hybrid_encrypt(curve.cid, s["st"], s["g"], s["esk"], pk, s["h"], s["t"])
    want = zb.hybrid_encrypt_host(curve.cid, s["st"], s["g"], s["esk"], pk, s["h"], s["t"])
    assert got[3].tolist() == want[3].tolist() and got[3][63] == 2 and eu.points_of(got[0][63])[0] == ID
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], want[:3]))


@CURVES
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_hybrid_device_pointers(backend, curve, shape):
    width, h, n = shape
    s = scan_batch(curve, shape)
    count = s["esk"].shape[0]
    d_esk, d_pk, d_h, d_t = dev(s["esk"]), dev(s["pk"]), dev(s["h"]) if h else None, dev(s["t"])
    d_epk, d_ct, d_tag, d_st = dev(np.zeros_like(s["epk"])), dev(np.zeros_like(s["ct"])), dev(np.zeros_like(s["tag"])), dev(np.zeros(count, dtype=np.uint8))
    hp = d_h.data_ptr() if h else 0
    backend.hybrid_encrypt_dev(curve.cid, width, s["st"], s["g"], d_esk.data_ptr(), d_pk.data_ptr(), 1, hp, h, d_t.data_ptr(), n, count, d_epk.data_ptr(), d_ct.data_ptr(),
                               d_tag.data_ptr(), d_st.data_ptr())
    assert host64(d_epk).tobytes() == s["epk"].tobytes() and host64(d_ct).tobytes() == s["ct"].tobytes() and host64(d_tag).tobytes() == s["tag"].tobytes()
    assert not d_st.cpu().numpy().any() and host64(d_t).tobytes() == s["t"].tobytes()
    d_sk, d_pt = dev(s["sk0"]), dev(np.zeros_like(s["t"]))
    ok = backend.hybrid_decrypt_dev(curve.cid, width, s["st"], d_sk.data_ptr(), 0, d_epk.data_ptr(), hp, h, d_ct.data_ptr(), d_tag.data_ptr(), n, count, d_pt.data_ptr(),
                                    d_st.data_ptr())
    assert np.flatnonzero(ok).tolist() == s["ours"] and not d_st.cpu().numpy().any()
    got = host64(d_pt).reshape(s["t"].shape)
    assert got[s["ours"]].tobytes() == s["t"][s["ours"]].tobytes()
    assert got.tobytes() == zb.hybrid_decrypt_host(curve.cid, s["st"], s["sk0"], s["epk"], s["h"], s["ct"], s["tag"])[0].tobytes()
