"""k_ed_hybrid_ladders (csrc/zl_edwards_dev.hip) and k_pos_duplex_trace_in (csrc/zl_poseidon_dev.hip): the assignments of the hybrid-encryption circuit written by
the device -- one lane per (row, ladder), then the cipher keyed from the row's own cells -- against the host mirror of the same entry point
(tests/test_hybrid_circuit_host.py pins that one to both host compilers and to the Python builder), byte for byte: both curves, bits 1, 2, 17 and full width at
(W; H, N) = (3; 0, 1) and bits 17 at (4; 1, 2), (5; 0, 1), (6; 3, 1); at the 64-lane workgroup edges and over three chunks of 64 rows; a sentinel row behind the
batch, a padded row stride, per-item keys and one shared key, edge scalars among the items, the staged host-pointer form, every refused item as one of 65, and
the public inputs against Backend.hybrid_encrypt -- k_ed_mul / k_ed_mul_fixed and k_pos_duplex, an independent kernel path."""
import numpy as np
import pytest

import edwards_util as eu
import hybrid_circuit_util as hu
import oracle_lib as ol
import poseidon_util as pu
from openzl_amd import BackendError, ed_order_bits, hybrid_encrypt_assignment_elems, hybrid_encrypt_assignments_host, load_library

pytestmark = pytest.mark.gpu
EINVAL = -1
COUNTS = (1, 63, 64, 65, 130)
N = 130
SENTINEL = 0xA5A5A5A5A5A5A5A5
SHAPES = [((3, 0, 1), 1), ((3, 0, 1), 2), ((3, 0, 1), 17), ((3, 0, 1), 0), ((4, 1, 2), 17), ((5, 0, 1), 17), ((6, 3, 1), 17)]  # bits 0: the full width
CASES = [(c, s, b) for c in pu.CURVES for s, b in SHAPES]
CASE = pytest.mark.parametrize("curve,shape,bits", CASES, ids=lambda v: getattr(v, "name", "-".join(map(str, v)) if isinstance(v, tuple) else str(v)))

_REF = {}


def ref(curve, shape, bits):
    """the operands of 130 items and the host mirror's rows, per-item keys and one shared key; public keys: the identity, points of order 2, 4 and 8, subgroup
    points and points of the full group in turn; the edge scalars that fit the width first and again around the first workgroup edge; computed once"""
    key = (curve.name, shape, bits)
    if key not in _REF:
        w, h, n = shape
        l = eu.params(curve)[3]
        width = bits or l.bit_length()
        top = min(l, 1 << width)
        pool = [eu.ID] + list(eu.small_order_points(curve)) + eu.subgroup_points(curve, 3, 41) + eu.random_points(curve, 3, 42)
        pks = [pool[i % len(pool)] for i in range(N)]
        edge = sorted({k for k in eu.edge_scalars(curve) if k < top} | {0, 1, top - 1})
        ks = [k % top for k in eu.random_scalars(curve, N, 43 + width)]
        ks[:len(edge)] = edge
        ks[64 - len(edge) // 2:64 - len(edge) // 2 + len(edge)] = edge
        ks = ks[:N]
        vals = pu.random_elems(curve, w + N * (h + n * (w - 1)), 44 + w)
        ops = dict(st=pu.limbs(vals[:w]), g=eu.point_words(eu.subgroup_points(curve, 1, 45))[0], esk=pu.limbs(ks), pk=eu.point_words(pks),
                   h=pu.limbs(vals[w:w + N * h]).reshape(N, h, 4), t=pu.limbs(vals[w + N * h:]).reshape(N, n, w - 1, 4))
        exp = hybrid_encrypt_assignments_host(curve.cid, ops["st"], ops["g"], ops["esk"], ops["pk"], ops["h"], ops["t"], width)
        shared = hybrid_encrypt_assignments_host(curve.cid, ops["st"], ops["g"], ops["esk"], ops["pk"][9], ops["h"], ops["t"], width)
        exp.setflags(write=False)
        shared.setflags(write=False)
        _REF[key] = (width, ops, exp, shared)
    return _REF[key]


def dev(a: np.ndarray):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def host(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(autouse=True)
def device_path(monkeypatch):
    monkeypatch.setenv("ZL_TUNE_ED_DEV_MIN", "0")
    monkeypatch.setenv("ZL_TUNE_ED_CHUNK", "64")
    return monkeypatch


@CASE
def test_rows_equal_the_host_mirror(backend, curve, shape, bits, device_path):
    width, o, exp, shared = ref(curve, shape, bits)
    w, h, n = shape
    nv = hybrid_encrypt_assignment_elems(curve.cid, w, width, h, n)
    assert width == (bits or ed_order_bits(curve.cid)) and exp.shape == (N, nv, 4) and nv == hu.row_elems(w, width, h, n)
    d_e, d_pk, d_h, d_t = dev(o["esk"]), dev(o["pk"]), dev(o["h"]), dev(o["t"])
    h_ptr = d_h.data_ptr() if h else 0

    def run(d_keys, ps, count, d_out, stride=None):
        backend.hybrid_encrypt_assignments_dev(curve.cid, w, width, o["st"], o["g"], d_e.data_ptr(), d_keys.data_ptr(), ps, h_ptr, h, d_t.data_ptr(), n, count, d_out.data_ptr(),
                                               stride)

    for count in COUNTS:  # one launch, a full block, a block and one lane, three chunks of 64
        d_out = dev(np.full((count + 1, nv, 4), SENTINEL, dtype=np.uint64))  # one spare row behind the batch
        run(d_pk, 1, count, d_out)
        out = host(d_out).reshape(count + 1, nv, 4)
        assert out[:count].tobytes() == exp[:count].tobytes(), count
        assert (out[count] == SENTINEL).all(), count
    run(d_pk, 1, 0, d_out)
    # one public key for all items
    d_one = dev(o["pk"][9])
    d_out = dev(np.full((N, nv, 4), SENTINEL, dtype=np.uint64))
    run(d_one, 0, N, d_out)
    assert host(d_out).reshape(N, nv, 4).tobytes() == shared.tobytes()
    # a padded stride: the words behind every row stay as they were
    stride = nv + 3
    d_out = dev(np.full((66, stride, 4), SENTINEL, dtype=np.uint64))
    run(d_pk, 1, 65, d_out, stride)
    out = host(d_out).reshape(66, stride, 4)
    assert out[:65, :nv].tobytes() == exp[:65].tobytes()
    assert (out[:65, nv:] == SENTINEL).all() and (out[65] == SENTINEL).all()
    # the staged host-pointer form, in chunks of 64 and in one
    assert backend.hybrid_encrypt_assignments(curve.cid, o["st"], o["g"], o["esk"], o["pk"], o["h"], o["t"], width).tobytes() == exp.tobytes()
    assert backend.hybrid_encrypt_assignments(curve.cid, o["st"], o["g"], o["esk"], o["pk"][9], o["h"], o["t"], width).tobytes() == shared.tobytes()
    device_path.delenv("ZL_TUNE_ED_CHUNK")
    assert backend.hybrid_encrypt_assignments(curve.cid, o["st"], o["g"], o["esk"], o["pk"], o["h"], o["t"], width).tobytes() == exp.tobytes()
    assert backend.hybrid_encrypt_assignments(curve.cid, o["st"], o["g"], o["esk"][:0], o["pk"][:0], o["h"][:0], o["t"][:0], width).shape == (0, nv, 4)


@CASE
def test_public_inputs_are_the_batched_encryption(backend, curve, shape, bits):
    width, o, exp, shared = ref(curve, shape, bits)
    w, h, n = shape
    t = n * (w - 1)
    epk, ct, tag, status = backend.hybrid_encrypt(curve.cid, o["st"], o["g"], o["esk"], o["pk"], o["h"], o["t"])
    assert not status.any()
    assert np.array_equal(exp[:, 0], np.tile(np.array([1, 0, 0, 0], dtype=np.uint64), (N, 1)))
    assert np.array_equal(exp[:, 1:3], np.tile(o["g"], (N, 1, 1))) and np.array_equal(exp[:, 3:5], o["pk"]) and np.array_equal(exp[:, 5:7], epk)
    assert np.array_equal(exp[:, 7], tag) and np.array_equal(exp[:, 8:8 + t], ct.reshape(N, t, 4)) and np.array_equal(exp[:, 8 + t:8 + t + h], o["h"])
    assert np.array_equal(exp[:, 8 + t + h], o["esk"])
    epk9, ct9, tag9, _ = backend.hybrid_encrypt(curve.cid, o["st"], o["g"], o["esk"], o["pk"][9], o["h"], o["t"])
    assert np.array_equal(shared[:, 5:7], epk9) and np.array_equal(shared[:, 7], tag9) and np.array_equal(shared[:, 8:8 + t], ct9.reshape(N, t, 4))


@pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
def test_errors(backend, curve, device_path):
    shape = (4, 1, 2)
    w, h, n = shape
    width, o, exp, _ = ref(curve, shape, 17)
    nv = exp.shape[1]
    count = 65
    fq, l = eu.params(curve)[0], eu.params(curve)[3]
    r = curve.fr.p
    x, y = eu.points_of(o["pk"][8])[0]
    d_out = dev(np.zeros((count, nv, 4), dtype=np.uint64))
    d_h, d_t = dev(o["h"]), dev(o["t"])
    for which in ("curve", "range", "wide", "order", "text"):  # one refused item among 65, in the second workgroup
        pp, kk, tt, bits = o["pk"][:count].copy(), o["esk"][:count].copy(), o["t"][:count].copy(), width
        if which == "curve":
            pp[64] = eu.point_words([(x, (y + 1) % fq)])[0]
        elif which == "range":
            pp[64] = eu.point_words([(fq, 1)])[0]
        elif which == "wide":
            kk[64] = pu.limbs([1 << 17])[0]
        elif which == "order":
            kk, bits = pu.limbs([1] * 64 + [l]), l.bit_length()
        else:
            tt[64, 1, 0] = pu.limbs([r])[0]
        d_bad_out = d_out if bits == width else dev(np.zeros((count, hybrid_encrypt_assignment_elems(curve.cid, w, bits, h, n), 4), dtype=np.uint64))
        d_pp, d_kk, d_tt = dev(pp), dev(kk), dev(tt)
        with pytest.raises(BackendError) as e:
            backend.hybrid_encrypt_assignments_dev(curve.cid, w, bits, o["st"], o["g"], d_kk.data_ptr(), d_pp.data_ptr(), 1, d_h.data_ptr(), h, d_tt.data_ptr(), n, count,
                                                   d_bad_out.data_ptr())
        assert e.value.code == EINVAL, which
        with pytest.raises(BackendError) as e:
            backend.hybrid_encrypt_assignments(curve.cid, o["st"], o["g"], kk, pp, o["h"][:count], tt, bits)
        assert e.value.code == EINVAL, which
    d_p, d_k = dev(o["pk"]), dev(o["esk"])
    for bits, stride, out_ptr, ps in ((width, nv - 1, d_out.data_ptr(), 1), (width, nv, d_out.data_ptr() + 8, 1), (0, nv, d_out.data_ptr(), 1),
                                      (l.bit_length() + 1, 27 * 253 + nv, d_out.data_ptr(), 1), (width, nv, d_out.data_ptr(), 2)):
        with pytest.raises(BackendError) as e:  # a short stride, a misaligned row, bits out of range, a key stride above 1
            backend._check(backend.L.zl_hybrid_encrypt_assignments_dev(backend._ctx, curve.cid, w, bits, ol.p64(o["st"]), ol.p64(o["g"]), d_k.data_ptr(), d_p.data_ptr(), ps,
                                                                       d_h.data_ptr(), h, d_t.data_ptr(), n, count, out_ptr, stride), "dev")
        assert e.value.code == EINVAL
    # the device-pointer form never takes the host path: a null ctx is refused
    out = np.zeros((1, nv, 4), dtype=np.uint64)
    assert load_library().zl_hybrid_encrypt_assignments_dev(None, curve.cid, w, width, ol.p64(o["st"]), ol.p64(o["g"]), ol.p64(o["esk"]), ol.p64(o["pk"]), 1, ol.p64(o["h"]), h,
                                                            ol.p64(o["t"]), n, 1, ol.p64(out), nv) == EINVAL
    # usable after the errors
    backend.hybrid_encrypt_assignments_dev(curve.cid, w, width, o["st"], o["g"], d_k.data_ptr(), d_p.data_ptr(), 1, d_h.data_ptr(), h, d_t.data_ptr(), n, count, d_out.data_ptr())
    assert host(d_out).reshape(count, nv, 4).tobytes() == exp[:count].tobytes()
