"""k_pos_duplex_trace (csrc/zl_poseidon_dev.hip): the assignments of the encryption circuit written by the device, against the host mirror of the same entry
point (tests/test_poseidon_encrypt_assignments_cpu.py pins that one to both host compilers and to the Python builder), byte for byte: every width and curve,
shapes A, B, C, F (and E at width 4) of that file, at the 64-lane workgroup edges and over more than four workgroups, with a padded row stride, over several
staged chunks, with the bound items, with an element at r, and the refusal of a null ctx by the device-pointer form."""
import numpy as np
import pytest

import oracle_lib as ol
import poseidon_duplex_util as du
import poseidon_util as pu
from openzl_amd import load_library, poseidon_encrypt_assignment_elems, poseidon_encrypt_assignments_host

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
WIDTHS = pytest.mark.parametrize("width", [3, 4, 5, 6])
EINVAL = -1
COUNTS = (1, 63, 64, 65, 257)
SENTINEL = 0xA5A5A5A5A5A5A5A5
N = 257

_REF = {}


def shapes(width):
    rate = width - 1
    out = {"A": (1, 0, 1), "B": (rate, 0, 1), "C": (rate + 1, 1, 2), "F": (2, rate, 1)}
    if width == 4:
        out["E"] = (2, 0, 1)
    return out


def ref(curve, width, name):
    """(initial state words or None, keys, headers, texts, the host mirror's rows) of 257 items: the bound items in the first lanes and around the first
    workgroup edge; the initial state is zero for shape A, a state with constant non-zero rate lanes for B and F, random otherwise"""
    key = (curve.name, width, name)
    if key not in _REF:
        shape = shapes(width)[name]
        items = du.random_items(curve, width, shape, N, 500 + 10 * width + ord(name))
        bound = du.bound_items(curve, width, shape)
        items[:len(bound)] = bound
        items[60:60 + len(bound)] = bound
        st = {"A": None, "B": [0] + [curve.fr.p - 1 - i for i in range(width - 1)], "F": [0] + [curve.fr.p - 1 - i for i in range(width - 1)]}.get(
            name, pu.random_elems(curve, width, 40 + width))
        stw = None if st is None else pu.limbs(st)
        k, h, t = du.pack(items, width, shape)
        exp = poseidon_encrypt_assignments_host(curve.cid, stw, k, h, t)
        exp.setflags(write=False)
        _REF[key] = (stw, k, h, t, exp)
    return _REF[key]


def dev(a: np.ndarray):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def dev_ops(k, h, t):
    """the operands in device memory; an empty header gets one element of backing so that its address is a device address"""
    return dev(k), dev(h if h.size else np.zeros((1, 4), dtype=np.uint64)), dev(t)


def host(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(autouse=True)
def device_path(monkeypatch):
    monkeypatch.setenv("ZL_TUNE_POSEIDON_DEV_MIN", "0")
    return monkeypatch


@CURVES
@WIDTHS
def test_rows_equal_the_host_mirror(backend, curve, width, device_path):
    for name, (kl, hl, n) in sorted(shapes(width).items()):
        stw, k, h, t, exp = ref(curve, width, name)
        nv = poseidon_encrypt_assignment_elems(width, kl, hl, n)
        assert exp.shape == (N, nv, 4)
        d_k, d_h, d_t = dev_ops(k, h, t)
        for count in COUNTS:
            d_out = dev(np.full((count + 1, nv, 4), SENTINEL, dtype=np.uint64))  # one spare row behind the batch
            backend.poseidon_encrypt_assignments_dev(curve.cid, width, stw, d_k.data_ptr(), kl, d_h.data_ptr(), hl, d_t.data_ptr(), n, count, d_out.data_ptr())
            out = host(d_out).reshape(count + 1, nv, 4)
            assert out[:count].tobytes() == exp[:count].tobytes(), (name, count)
            assert (out[count] == SENTINEL).all(), (name, count)
            got = backend.poseidon_encrypt_assignments(curve.cid, stw, k[:count], h[:count], t[:count])
            assert got.shape == (count, nv, 4) and got.tobytes() == exp[:count].tobytes(), (name, count)
        assert backend.poseidon_encrypt_assignments(curve.cid, stw, k[:0], h[:0], t[:0]).shape == (0, nv, 4)
        backend.poseidon_encrypt_assignments_dev(curve.cid, width, stw, d_k.data_ptr(), kl, d_h.data_ptr(), hl, d_t.data_ptr(), n, 0, d_out.data_ptr())
        # a padded stride: the words behind every row stay as they were
        stride = nv + 3
        d_out = dev(np.full((N + 1, stride, 4), SENTINEL, dtype=np.uint64))
        backend.poseidon_encrypt_assignments_dev(curve.cid, width, stw, d_k.data_ptr(), kl, d_h.data_ptr(), hl, d_t.data_ptr(), n, N, d_out.data_ptr(), stride)
        out = host(d_out).reshape(N + 1, stride, 4)
        assert out[:N, :nv].tobytes() == exp.tobytes(), name
        assert (out[:N, nv:] == SENTINEL).all() and (out[N] == SENTINEL).all(), name
        # several staged chunks: 8 x 32 + 1
        device_path.setenv("ZL_TUNE_POSEIDON_CHUNK", "32")
        assert backend.poseidon_encrypt_assignments(curve.cid, stw, k, h, t).tobytes() == exp.tobytes(), name
        d_out = dev(np.full((N + 1, stride, 4), SENTINEL, dtype=np.uint64))
        backend.poseidon_encrypt_assignments_dev(curve.cid, width, stw, d_k.data_ptr(), kl, d_h.data_ptr(), hl, d_t.data_ptr(), n, N, d_out.data_ptr(), stride)
        out = host(d_out).reshape(N + 1, stride, 4)
        assert out[:N, :nv].tobytes() == exp.tobytes() and (out[:N, nv:] == SENTINEL).all() and (out[N] == SENTINEL).all(), name
        device_path.delenv("ZL_TUNE_POSEIDON_CHUNK")


@CURVES
def test_errors(backend, curve, device_path):
    from openzl_amd import BackendError

    width, name = 4, "C"
    kl, hl, n = shapes(width)[name]
    stw, k, h, t, exp = ref(curve, width, name)
    nv = exp.shape[1]
    count = 70
    at_r = pu.limbs([curve.fr.p])[0]
    d_out = dev(np.zeros((count, nv, 4), dtype=np.uint64))
    for which in ("key", "header", "text"):  # an element at r in device memory, in the second workgroup
        ops = [k[:count].copy(), h[:count].copy(), t[:count].copy()]
        if which == "key":
            ops[0][66, kl - 1] = at_r
        elif which == "header":
            ops[1][66, 0] = at_r
        else:
            ops[2][66, n - 1, width - 2] = at_r
        d_k, d_h, d_t = dev_ops(*ops)
        with pytest.raises(BackendError) as e:
            backend.poseidon_encrypt_assignments_dev(curve.cid, width, stw, d_k.data_ptr(), kl, d_h.data_ptr(), hl, d_t.data_ptr(), n, count, d_out.data_ptr())
        assert e.value.code == EINVAL, which
        with pytest.raises(BackendError) as e:
            backend.poseidon_encrypt_assignments(curve.cid, stw, *ops)
        assert e.value.code == EINVAL, which
    d_k, d_h, d_t = dev_ops(k[:count], h[:count], t[:count])
    bad_st = stw.copy()
    bad_st[width - 1] = at_r
    for stride, out_ptr, st in ((nv - 1, d_out.data_ptr(), stw), (nv, d_out.data_ptr() + 8, stw), (nv, d_out.data_ptr(), bad_st)):  # a short stride, a misaligned row, a state at r
        with pytest.raises(BackendError) as e:
            backend.poseidon_encrypt_assignments_dev(curve.cid, width, st, d_k.data_ptr(), kl, d_h.data_ptr(), hl, d_t.data_ptr(), n, count, out_ptr, stride)
        assert e.value.code == EINVAL
    # the device-pointer form never takes the host path: a null ctx is refused
    p64 = ol.p64
    out = np.zeros((1, nv, 4), dtype=np.uint64)
    assert load_library().zl_poseidon_encrypt_assignments_dev(None, curve.cid, width, p64(stw), p64(k), kl, p64(h), hl, p64(t), n, 1, p64(out), nv) == EINVAL
    # usable after the errors
    backend.poseidon_encrypt_assignments_dev(curve.cid, width, stw, d_k.data_ptr(), kl, d_h.data_ptr(), hl, d_t.data_ptr(), n, count, d_out.data_ptr())
    assert host(d_out).reshape(count, nv, 4).tobytes() == exp[:count].tobytes()
