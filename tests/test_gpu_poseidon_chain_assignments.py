"""k_pos_chain_trace (csrc/zl_poseidon_dev.hip): the assignments of Poseidon-chain circuits written by the device, against the host path of the same entry point
(tests/test_poseidon_chain_assignments_cpu.py pins that one to both host compilers), at the 64-lane workgroup edges, with a padded row stride, over several
launches, on either side of the host / device threshold, on a foreign stream and with a non-canonical input."""
import numpy as np
import pytest

import poseidon_util as pu
from openzl_amd import poseidon_chain_assignment_elems, poseidon_chain_assignments_host
from openzl_amd import backend as zb

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
EINVAL = -1
HUGE = str(1 << 30)
COUNTS = (1, 63, 64, 65, 130)
SENTINEL = 0xA5A5A5A5A5A5A5A5

_REF = {}


def ref(curve, k):
    """130 chains (0 / r - 1 / 1 in the first lanes, then random) with the host path's assignments, computed once per (curve, k) and shared"""
    if (curve.name, k) not in _REF:
        r = curve.fr.p
        x0, x1 = pu.random_elems(curve, 130, 411), pu.random_elems(curve, 130, 412)
        x0[:3], x1[:3] = [0, r - 1, 1], [0, r - 1, 2]
        a, b = pu.limbs(x0), pu.limbs(x1)
        exp = poseidon_chain_assignments_host(curve.cid, a, b, k)
        exp.setflags(write=False)
        _REF[(curve.name, k)] = (a, b, exp)
    return _REF[(curve.name, k)]


def dev(a: np.ndarray):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def host(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(autouse=True)
def device_path(monkeypatch):
    monkeypatch.setenv("ZL_TUNE_POSEIDON_DEV_MIN", "0")
    return monkeypatch


@CURVES
@pytest.mark.parametrize("k", [1, 2, 3])
def test_device_rows_equal_the_host_path_at_workgroup_edges(backend, curve, k):
    a, b, exp = ref(curve, k)
    nv = poseidon_chain_assignment_elems(k)
    for count in COUNTS:
        got = backend.poseidon_chain_assignments(curve.cid, a[:count], b[:count], k)
        assert got.shape == (count, nv, 4)
        assert got.tobytes() == exp[:count].tobytes(), count
    assert backend.poseidon_chain_assignments(curve.cid, a[:0], b[:0], k).shape == (0, nv, 4)


@CURVES
@pytest.mark.parametrize("k", [1, 2, 3])
def test_device_pointers_with_a_padded_stride_leave_the_padding_alone(backend, curve, k):
    a, b, exp = ref(curve, k)
    nv = poseidon_chain_assignment_elems(k)
    stride = nv + 5
    d_a, d_b = dev(a), dev(b)
    for count in COUNTS:
        d_out = dev(np.full((count + 1, stride, 4), SENTINEL, dtype=np.uint64))  # one spare row behind the batch
        backend.poseidon_chain_assignments_dev(curve.cid, d_a.data_ptr(), d_b.data_ptr(), k, count, d_out.data_ptr(), stride)
        out = host(d_out).reshape(count + 1, stride, 4)
        assert out[:count, :nv].tobytes() == exp[:count].tobytes(), count
        assert (out[:count, nv:] == SENTINEL).all() and (out[count] == SENTINEL).all(), count
    d_out = dev(np.full((130, nv, 4), SENTINEL, dtype=np.uint64))
    backend.poseidon_chain_assignments_dev(curve.cid, d_a.data_ptr(), d_b.data_ptr(), k, 130, d_out.data_ptr())  # default: dense rows
    assert host(d_out).tobytes() == exp.tobytes()
    backend.poseidon_chain_assignments_dev(curve.cid, d_a.data_ptr(), d_b.data_ptr(), k, 0, d_out.data_ptr())
    for bad_stride, ptr in ((nv - 1, d_out.data_ptr()), (nv, d_out.data_ptr() + 8)):  # a stride below the row, a destination off 16 bytes
        with pytest.raises(zb.BackendError) as e:
            backend.poseidon_chain_assignments_dev(curve.cid, d_a.data_ptr(), d_b.data_ptr(), k, 2, ptr, bad_stride)
        assert e.value.code == EINVAL


@CURVES
def test_three_launches_and_three_staged_chunks(backend, curve, device_path):
    device_path.setenv("ZL_TUNE_POSEIDON_CHUNK", "48")  # 48 + 48 + 34 chains
    a, b, exp = ref(curve, 2)
    assert backend.poseidon_chain_assignments(curve.cid, a, b, 2).tobytes() == exp.tobytes()
    d_a, d_b, d_out = dev(a), dev(b), dev(np.zeros((130, 472, 4), dtype=np.uint64))
    backend.poseidon_chain_assignments_dev(curve.cid, d_a.data_ptr(), d_b.data_ptr(), 2, 130, d_out.data_ptr())
    assert host(d_out).tobytes() == exp.tobytes()


@CURVES
def test_host_and_device_side_of_the_threshold_agree(backend, curve, device_path):
    a, b, exp = ref(curve, 3)
    on_dev = backend.poseidon_chain_assignments(curve.cid, a[:65], b[:65], 3)
    device_path.setenv("ZL_TUNE_POSEIDON_DEV_MIN", HUGE)
    on_host = backend.poseidon_chain_assignments(curve.cid, a[:65], b[:65], 3)
    assert on_dev.tobytes() == on_host.tobytes() == exp[:65].tobytes()


@CURVES
def test_foreign_stream_and_forked_lane(backend, curve):
    import torch

    a, b, exp = ref(curve, 1)
    lane = backend.fork()
    try:
        assert lane.poseidon_chain_assignments(curve.cid, a, b, 1).tobytes() == exp.tobytes()
    finally:
        lane.close()
        backend._forks.remove(lane)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        backend.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            d_a = torch.from_numpy(a.view(np.int64).copy()).cuda()
            d_b = torch.from_numpy(b.view(np.int64).copy()).cuda()
            d_out = torch.zeros(130 * 238 * 4, dtype=torch.int64, device="cuda")
            backend.poseidon_chain_assignments_dev(curve.cid, d_a.data_ptr(), d_b.data_ptr(), 1, 130, d_out.data_ptr())
            assert host(d_out).tobytes() == exp.tobytes()
            assert backend.poseidon_chain_assignments(curve.cid, a, b, 1).tobytes() == exp.tobytes()
        finally:
            backend.set_stream(0)


@CURVES
def test_non_canonical_input_in_the_middle_is_refused_and_the_ctx_lives_on(backend, curve, device_path):
    a, b, exp = ref(curve, 1)
    for which, value in ((0, curve.fr.p), (1, (1 << 256) - 1)):
        bad = [a.copy(), b.copy()]
        bad[which][70] = pu.limbs([value])[0]
        with pytest.raises(zb.BackendError) as e:
            backend.poseidon_chain_assignments(curve.cid, bad[0], bad[1], 1)
        assert e.value.code == EINVAL
        d_a, d_b, d_out = dev(bad[0]), dev(bad[1]), dev(np.zeros((130, 238, 4), dtype=np.uint64))
        with pytest.raises(zb.BackendError) as e:
            backend.poseidon_chain_assignments_dev(curve.cid, d_a.data_ptr(), d_b.data_ptr(), 1, 130, d_out.data_ptr())
        assert e.value.code == EINVAL
    device_path.setenv("ZL_TUNE_POSEIDON_CHUNK", "48")  # ... in the second of three chunks
    with pytest.raises(zb.BackendError) as e:
        backend.poseidon_chain_assignments(curve.cid, bad[0], bad[1], 1)
    assert e.value.code == EINVAL
    assert backend.poseidon_chain_assignments(curve.cid, a, b, 1).tobytes() == exp.tobytes()  # the flag does not stick
    with pytest.raises(zb.BackendError) as e:
        backend.poseidon_chain_assignments(curve.cid, a[:2], b[:2], 0)
    assert e.value.code == EINVAL
