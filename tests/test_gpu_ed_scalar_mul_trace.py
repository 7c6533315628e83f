"""k_ed_mul_trace (csrc/zl_edwards_dev.hip): the assignments of the scalar-multiplication circuit written by the device, against the host mirror of the same
entry point (tests/test_ed_circuit_host.py pins that one to both host compilers and to the Python builder), byte for byte: both curves at bits 1, 2, 17 and
full width, at the 64-lane workgroup edges and over several chunks of 64 rows, per-item points and one shared point, edge scalars among the items, a padded
row stride, the staged host-pointer form, an off-curve point among 65, and the public inputs against zl_ed_scalar_mul_batch."""
import numpy as np
import pytest

import edwards_util as eu
import oracle_lib as ol
import poseidon_util as pu
from openzl_amd import BackendError, ed_order_bits, ed_scalar_mul_assignment_elems, ed_scalar_mul_assignments_host, ed_scalar_mul_host, load_library

pytestmark = pytest.mark.gpu
EINVAL = -1
COUNTS = (1, 63, 64, 65, 130)
N = 130
SENTINEL = 0xA5A5A5A5A5A5A5A5
CASES = [(c, b) for c in pu.CURVES for b in (1, 2, 17, 0)]  # 0: the full width
CASE = pytest.mark.parametrize("curve,bits", CASES, ids=lambda v: getattr(v, "name", str(v)))

_REF = {}


def ref(curve, bits):
    """(bits, points (N, 2, 4), scalars (N, 4), the host mirror's rows, the rows of one shared point) of 130 items: the identity, points of order 2, 4 and 8,
    subgroup points and points of the full group in turn; the edge scalars that fit the width first and again around the first workgroup edge; computed once"""
    key = (curve.name, bits)
    if key not in _REF:
        l = eu.params(curve)[3]
        width = bits or l.bit_length()
        top = min(l, 1 << width)
        pool = [eu.ID] + list(eu.small_order_points(curve)) + eu.subgroup_points(curve, 3, 31) + eu.random_points(curve, 3, 32)
        pts = [pool[i % len(pool)] for i in range(N)]
        edge = sorted({k for k in eu.edge_scalars(curve) if k < top} | {0, 1, top - 1})
        ks = [k % top for k in eu.random_scalars(curve, N, 33 + width)]
        ks[:len(edge)] = edge
        ks[64 - len(edge) // 2:64 - len(edge) // 2 + len(edge)] = edge
        ks = ks[:N]
        p, k = eu.point_words(pts), pu.limbs(ks)
        exp = ed_scalar_mul_assignments_host(curve.cid, p, k, width)
        shared = ed_scalar_mul_assignments_host(curve.cid, p[9], k, width)
        exp.setflags(write=False)
        shared.setflags(write=False)
        _REF[key] = (width, p, k, exp, shared)
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
def test_rows_equal_the_host_mirror(backend, curve, bits, device_path):
    width, p, k, exp, shared = ref(curve, bits)
    nv = ed_scalar_mul_assignment_elems(curve.cid, width)
    assert width == (bits or ed_order_bits(curve.cid)) and exp.shape == (N, nv, 4) and nv == 14 * width - 5
    d_p, d_k = dev(p), dev(k)
    for count in COUNTS:  # one launch, a full block, a block and one lane, three chunks of 64
        d_out = dev(np.full((count + 1, nv, 4), SENTINEL, dtype=np.uint64))  # one spare row behind the batch
        backend.ed_scalar_mul_assignments_dev(curve.cid, width, d_p.data_ptr(), 1, d_k.data_ptr(), count, d_out.data_ptr())
        out = host(d_out).reshape(count + 1, nv, 4)
        assert out[:count].tobytes() == exp[:count].tobytes(), count
        assert (out[count] == SENTINEL).all(), count
    backend.ed_scalar_mul_assignments_dev(curve.cid, width, d_p.data_ptr(), 1, d_k.data_ptr(), 0, d_out.data_ptr())
    # one point for all items
    d_one = dev(p[9])
    d_out = dev(np.full((N, nv, 4), SENTINEL, dtype=np.uint64))
    backend.ed_scalar_mul_assignments_dev(curve.cid, width, d_one.data_ptr(), 0, d_k.data_ptr(), N, d_out.data_ptr())
    assert host(d_out).reshape(N, nv, 4).tobytes() == shared.tobytes()
    # a padded stride: the words behind every row stay as they were
    stride = nv + 3
    d_out = dev(np.full((66, stride, 4), SENTINEL, dtype=np.uint64))
    backend.ed_scalar_mul_assignments_dev(curve.cid, width, d_p.data_ptr(), 1, d_k.data_ptr(), 65, d_out.data_ptr(), stride)
    out = host(d_out).reshape(66, stride, 4)
    assert out[:65, :nv].tobytes() == exp[:65].tobytes()
    assert (out[:65, nv:] == SENTINEL).all() and (out[65] == SENTINEL).all()
    # the staged host-pointer form, in chunks of 64 and in one
    assert backend.ed_scalar_mul_assignments(curve.cid, p, k, width).tobytes() == exp.tobytes()
    assert backend.ed_scalar_mul_assignments(curve.cid, p[9], k, width).tobytes() == shared.tobytes()
    device_path.delenv("ZL_TUNE_ED_CHUNK")
    assert backend.ed_scalar_mul_assignments(curve.cid, p, k, width).tobytes() == exp.tobytes()
    assert backend.ed_scalar_mul_assignments(curve.cid, p[:0], k[:0], width).shape == (0, nv, 4)


@CASE
def test_public_inputs_are_the_batched_multiplication(backend, curve, bits):
    width, p, k, exp, shared = ref(curve, bits)
    q, status = backend.ed_scalar_mul(curve.cid, p, k)
    assert not status.any()
    assert np.array_equal(exp[:, 0], np.tile(np.array([1, 0, 0, 0], dtype=np.uint64), (N, 1)))
    assert np.array_equal(exp[:, 1:3], p) and np.array_equal(exp[:, 3:5], q) and np.array_equal(exp[:, 5], k)
    q9, _ = ed_scalar_mul_host(curve.cid, p[9], k)
    assert np.array_equal(shared[:, 3:5], q9)


@pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
def test_errors(backend, curve, device_path):
    width, p, k, exp, _ = ref(curve, 17)
    nv = exp.shape[1]
    count = 65
    fq, l = eu.params(curve)[0], eu.params(curve)[3]
    x, y = eu.points_of(p[8])[0]
    d_out = dev(np.zeros((count, nv, 4), dtype=np.uint64))
    d_k = dev(k)
    for which in ("curve", "range", "wide", "order"):  # one refused item among 65, in the second workgroup
        pp, kk, bits = p[:count].copy(), k[:count].copy(), width
        if which == "curve":
            pp[64] = eu.point_words([(x, (y + 1) % fq)])[0]
        elif which == "range":
            pp[64] = eu.point_words([(fq, 1)])[0]
        elif which == "wide":
            kk[64] = pu.limbs([1 << 17])[0]
        else:
            kk, bits = pu.limbs([1] * 64 + [l]), l.bit_length()
        d_bad_out = d_out if bits == width else dev(np.zeros((count, ed_scalar_mul_assignment_elems(curve.cid, bits), 4), dtype=np.uint64))
        d_pp, d_kk = dev(pp), dev(kk)
        with pytest.raises(BackendError) as e:
            backend.ed_scalar_mul_assignments_dev(curve.cid, bits, d_pp.data_ptr(), 1, d_kk.data_ptr(), count, d_bad_out.data_ptr())
        assert e.value.code == EINVAL, which
        with pytest.raises(BackendError) as e:
            backend.ed_scalar_mul_assignments(curve.cid, pp, kk, bits)
        assert e.value.code == EINVAL, which
    d_p = dev(p)
    for bits, stride, out_ptr, ps in ((width, nv - 1, d_out.data_ptr(), 1), (width, nv, d_out.data_ptr() + 8, 1), (0, nv, d_out.data_ptr(), 1),
                                      (l.bit_length() + 1, 14 * 253, d_out.data_ptr(), 1), (width, nv, d_out.data_ptr(), 2)):
        with pytest.raises(BackendError) as e:  # a short stride, a misaligned row, bits out of range, a point stride above 1
            backend._check(backend.L.zl_ed_scalar_mul_assignments_dev(backend._ctx, curve.cid, bits, d_p.data_ptr(), ps, d_k.data_ptr(), count, out_ptr, stride), "dev")
        assert e.value.code == EINVAL
    # the device-pointer form never takes the host path: a null ctx is refused
    out = np.zeros((1, nv, 4), dtype=np.uint64)
    assert load_library().zl_ed_scalar_mul_assignments_dev(None, curve.cid, width, ol.p64(p), 1, ol.p64(k), 1, ol.p64(out), nv) == EINVAL
    # usable after the errors
    backend.ed_scalar_mul_assignments_dev(curve.cid, width, d_p.data_ptr(), 1, d_k.data_ptr(), count, d_out.data_ptr())
    assert host(d_out).reshape(count, nv, 4).tobytes() == exp[:count].tobytes()
