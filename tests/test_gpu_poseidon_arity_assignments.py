"""k_pos_hash_trace / k_pos_leaf_merkle_trace (csrc/zl_poseidon_dev.hip): the assignments of the arity-general circuits written by the device, against the host
mirror of the same entry points (tests/test_poseidon_arity_assignments_cpu.py pins that one to both host compilers and to the Python builder): at the 64-lane
workgroup edges, with a padded row stride, over several staged chunks, with 0 and r - 1 in every input position, with an input at r, and read out of a tree
built on the device from its leaves' preimages -- where a preimage that does not hash to its leaf is refused."""
import numpy as np
import pytest

import poseidon_arity_util as pa
import poseidon_util as pu
from openzl_amd import (poseidon_chain_assignments_host, poseidon_hash_assignment_elems, poseidon_hash_assignments_host, poseidon_merkle_leaf_assignment_elems,
                        poseidon_merkle_leaf_assignments_host, poseidon_merkle_nodes)
from openzl_amd import backend as zb

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
ARITIES = pytest.mark.parametrize("arity", pa.ARITIES)
EINVAL = -1
COUNTS = (1, 63, 64, 65, 130)
SENTINEL = 0xA5A5A5A5A5A5A5A5
N = 130

_REF = {}


def inputs_of(curve, arity):
    """130 x arity elements: 0 and r - 1 in every position, in the first lanes and in the lanes around the workgroup edge"""
    r = curve.fr.p
    xs = np.array(pu.random_elems(curve, N * arity, 700 + arity), dtype=object).reshape(N, arity)
    for base in (0, 56, 120):
        for pos in range(arity):
            xs[base + 2 * pos, pos], xs[base + 2 * pos + 1, pos] = 0, r - 1
    return pu.limbs(xs.reshape(-1)).reshape(N, arity, 4)


def hash_ref(curve, arity):
    key = (curve.name, arity)
    if key not in _REF:
        v = inputs_of(curve, arity)
        exp = poseidon_hash_assignments_host(curve.cid, v)
        exp.setflags(write=False)
        _REF[key] = (v, exp)
    return _REF[key]


def leaf_ref(curve, arity, depth):
    key = (curve.name, arity, depth)
    if key not in _REF:
        rng = np.random.default_rng(800 + depth)
        pre = inputs_of(curve, arity)
        paths = np.array(pu.random_elems(curve, N * depth, 820 + arity + depth), dtype=object).reshape(N, depth)
        idx = [int(rng.integers(0, 1 << depth)) for _ in range(N)]
        for base in (0, 62, 127):
            idx[base], idx[base + 1] = 0, (1 << depth) - 1
            paths[base + 2, 0] = 0
            paths[base + 1, depth - 1] = 0
        pav = pu.limbs(paths.reshape(-1)).reshape(N, depth, 4)
        ix = np.array(idx, dtype=np.uint64)
        exp = poseidon_merkle_leaf_assignments_host(curve.cid, pre, ix, pav, depth)
        exp.setflags(write=False)
        _REF[key] = (pre, ix, pav, exp)
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
    monkeypatch.setenv("ZL_TUNE_POSEIDON_DEV_MIN", "0")
    return monkeypatch


@CURVES
@ARITIES
def test_hash_rows_equal_the_host_mirror(backend, curve, arity, device_path):
    v, exp = hash_ref(curve, arity)
    nv = poseidon_hash_assignment_elems(arity)
    d_in = dev(v)
    for count in COUNTS:
        d_out = dev(np.full((count + 1, nv, 4), SENTINEL, dtype=np.uint64))  # one spare row behind the batch
        backend.poseidon_hash_assignments_dev(curve.cid, arity, d_in.data_ptr(), count, d_out.data_ptr())
        out = host(d_out).reshape(count + 1, nv, 4)
        assert out[:count].tobytes() == exp[:count].tobytes(), count
        assert (out[count] == SENTINEL).all(), count
        got = backend.poseidon_hash_assignments(curve.cid, v[:count])
        assert got.shape == (count, nv, 4) and got.tobytes() == exp[:count].tobytes(), count
    assert backend.poseidon_hash_assignments(curve.cid, v[:0]).shape == (0, nv, 4)
    backend.poseidon_hash_assignments_dev(curve.cid, arity, d_in.data_ptr(), 0, d_out.data_ptr())
    # a padded stride: the words behind every row stay as they were
    stride = nv + 3
    d_out = dev(np.full((N + 1, stride, 4), SENTINEL, dtype=np.uint64))
    backend.poseidon_hash_assignments_dev(curve.cid, arity, d_in.data_ptr(), N, d_out.data_ptr(), stride)
    out = host(d_out).reshape(N + 1, stride, 4)
    assert out[:N, :nv].tobytes() == exp.tobytes()
    assert (out[:N, nv:] == SENTINEL).all() and (out[N] == SENTINEL).all()
    # several staged chunks: 32 + 32 + 32 + 32 + 2
    device_path.setenv("ZL_TUNE_POSEIDON_CHUNK", "32")
    assert backend.poseidon_hash_assignments(curve.cid, v).tobytes() == exp.tobytes()
    backend.poseidon_hash_assignments_dev(curve.cid, arity, d_in.data_ptr(), N, d_out.data_ptr(), stride)
    assert host(d_out).reshape(N + 1, stride, 4)[:N, :nv].tobytes() == exp.tobytes()
    device_path.delenv("ZL_TUNE_POSEIDON_CHUNK")
    if arity == 2:  # the row of a one-link chain, byte for byte
        assert exp.tobytes() == poseidon_chain_assignments_host(curve.cid, np.ascontiguousarray(v[:, 0]), np.ascontiguousarray(v[:, 1]), 1).tobytes()
    # an input at r, in the second workgroup; bad arguments; and the flag does not stick
    bad = v.copy()
    bad[70, arity - 1] = pu.limbs([curve.fr.p])[0]
    with pytest.raises(zb.BackendError) as e:
        backend.poseidon_hash_assignments(curve.cid, bad)
    assert e.value.code == EINVAL
    d_bad = dev(bad)
    with pytest.raises(zb.BackendError) as e:
        backend.poseidon_hash_assignments_dev(curve.cid, arity, d_bad.data_ptr(), N, d_out.data_ptr(), stride)
    assert e.value.code == EINVAL
    for bad_stride, ptr in ((nv - 1, d_out.data_ptr()), (stride, d_out.data_ptr() + 8)):  # a stride below the row, a destination off 16 bytes
        with pytest.raises(zb.BackendError) as e:
            backend.poseidon_hash_assignments_dev(curve.cid, arity, d_in.data_ptr(), 2, ptr, bad_stride)
        assert e.value.code == EINVAL
    assert backend.poseidon_hash_assignments(curve.cid, v[:65]).tobytes() == exp[:65].tobytes()


@CURVES
@ARITIES
@pytest.mark.parametrize("depth", [1, 3])
def test_leaf_membership_rows_from_explicit_paths(backend, curve, arity, depth, device_path):
    pre, ix, pav, exp = leaf_ref(curve, arity, depth)
    nv = poseidon_merkle_leaf_assignment_elems(arity, depth)
    assert nv == exp.shape[1]
    d_pre, d_pa = dev(pre), dev(pav)
    stride = nv + 3
    for count in COUNTS:
        d_out = dev(np.full((count + 1, stride, 4), SENTINEL, dtype=np.uint64))
        backend.poseidon_merkle_leaf_assignments_dev(curve.cid, arity, d_pre.data_ptr(), ix[:count], d_pa.data_ptr(), depth, d_out.data_ptr(), stride)
        out = host(d_out).reshape(count + 1, stride, 4)
        assert out[:count, :nv].tobytes() == exp[:count].tobytes(), count
        assert (out[:count, nv:] == SENTINEL).all() and (out[count] == SENTINEL).all(), count
    assert backend.poseidon_merkle_leaf_assignments(curve.cid, pre[:65], ix[:65], pav[:65], depth).tobytes() == exp[:65].tobytes()
    device_path.setenv("ZL_TUNE_POSEIDON_CHUNK", "32")
    assert backend.poseidon_merkle_leaf_assignments(curve.cid, pre, ix, pav, depth).tobytes() == exp.tobytes()
    d_out = dev(np.zeros((N, nv, 4), dtype=np.uint64))
    backend.poseidon_merkle_leaf_assignments_dev(curve.cid, arity, d_pre.data_ptr(), ix, d_pa.data_ptr(), depth, d_out.data_ptr())  # default: dense rows
    assert host(d_out).tobytes() == exp.tobytes()
    device_path.delenv("ZL_TUNE_POSEIDON_CHUNK")
    for which in ("preimage", "sibling"):
        bad_pre, bad_pa = pre.copy(), pav.copy()
        if which == "preimage":
            bad_pre[70, 0] = pu.limbs([curve.fr.p])[0]
        else:
            bad_pa[70, depth - 1] = pu.limbs([curve.fr.p])[0]
        with pytest.raises(zb.BackendError) as e:
            backend.poseidon_merkle_leaf_assignments(curve.cid, bad_pre, ix, bad_pa, depth)
        assert e.value.code == EINVAL
    bad_ix = ix[:2].copy()
    bad_ix[1] = 1 << depth
    for bad_stride, ptr, idx in ((nv - 1, d_out.data_ptr(), ix[:2]), (nv, d_out.data_ptr() + 8, ix[:2]), (nv, d_out.data_ptr(), bad_ix)):
        with pytest.raises(zb.BackendError) as e:
            backend.poseidon_merkle_leaf_assignments_dev(curve.cid, arity, d_pre.data_ptr(), idx, d_pa.data_ptr(), depth, ptr, bad_stride)
        assert e.value.code == EINVAL
    assert backend.poseidon_merkle_leaf_assignments(curve.cid, pre[:2], ix[:2], pav[:2], depth).tobytes() == exp[:2].tobytes()


@CURVES
@ARITIES
def test_leaf_memberships_out_of_a_device_tree(backend, curve, arity):
    """a 5-leaf tree of depth 3 (leaf 4 has absent siblings at levels 0 and 1), its leaves hashed on the device from their preimages: the member form's rows are
    the paths form's over the gathered paths, [1] of every row is the tree's root, and a preimage that does not hash to its leaf is refused"""
    n, depth = 5, 3
    pre = inputs_of(curve, arity)[:n].copy()
    d_pre = dev(pre)
    d_leaves = dev(np.zeros((n, 4), dtype=np.uint64))
    backend.poseidon_hash_dev(curve.cid, arity, d_pre.data_ptr(), n, d_leaves.data_ptr())
    d_nodes = dev(np.zeros((poseidon_merkle_nodes(n, depth), 4), dtype=np.uint64))
    root = backend.poseidon_merkle_build_dev(curve.cid, d_leaves.data_ptr(), n, depth, d_nodes.data_ptr())
    ix = np.array([4, 0, 3, 1, 2, 4], dtype=np.uint64)
    paths = backend.poseidon_merkle_paths(curve.cid, d_nodes.data_ptr(), n, depth, ix)
    assert not paths[0, 0].any() and not paths[0, 1].any() and paths[0, 2].any()
    exp = poseidon_merkle_leaf_assignments_host(curve.cid, pre[ix.astype(np.int64)], ix, paths, depth)
    nv = poseidon_merkle_leaf_assignment_elems(arity, depth)
    stride = nv + 3
    d_out = dev(np.full((ix.size + 1, stride, 4), SENTINEL, dtype=np.uint64))
    backend.poseidon_merkle_leaf_member_assignments_dev(curve.cid, arity, d_nodes.data_ptr(), d_pre.data_ptr(), n, depth, ix, d_out.data_ptr(), stride)
    out = host(d_out).reshape(ix.size + 1, stride, 4)
    assert out[:ix.size, :nv].tobytes() == exp.tobytes()
    assert (out[:ix.size, nv:] == SENTINEL).all() and (out[ix.size] == SENTINEL).all()
    assert np.array_equal(out[:ix.size, 1], np.tile(root, (ix.size, 1)))
    for bad in (n, 1 << depth):
        with pytest.raises(zb.BackendError) as e:
            backend.poseidon_merkle_leaf_member_assignments_dev(curve.cid, arity, d_nodes.data_ptr(), d_pre.data_ptr(), n, depth, np.array([0, bad], dtype=np.uint64),
                                                                d_out.data_ptr(), stride)
        assert e.value.code == EINVAL
    with pytest.raises(zb.BackendError) as e:  # more leaves than the depth holds
        backend.poseidon_merkle_leaf_member_assignments_dev(curve.cid, arity, d_nodes.data_ptr(), d_pre.data_ptr(), (1 << depth) + 1, depth, ix[:1], d_out.data_ptr(), stride)
    assert e.value.code == EINVAL
    wrong = pre.copy()
    wrong[3, 0, 0] ^= np.uint64(1)  # another canonical value as the first element of leaf 3's preimage (a random one: row 3 has its edge value at position 1)
    assert pu.ints(wrong[3, 0])[0] < curve.fr.p
    d_wrong = dev(wrong)
    with pytest.raises(zb.BackendError) as e:
        backend.poseidon_merkle_leaf_member_assignments_dev(curve.cid, arity, d_nodes.data_ptr(), d_wrong.data_ptr(), n, depth, ix, d_out.data_ptr(), stride)
    assert e.value.code == EINVAL
    # the items that do not touch leaf 3 pass with the same preimages, and the flag does not stick
    backend.poseidon_merkle_leaf_member_assignments_dev(curve.cid, arity, d_nodes.data_ptr(), d_wrong.data_ptr(), n, depth, ix[:2], d_out.data_ptr(), stride)
    assert host(d_out).reshape(ix.size + 1, stride, 4)[:2, :nv].tobytes() == exp[:2].tobytes()
