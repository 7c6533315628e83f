"""k_pos_merkle_trace (csrc/zl_poseidon_dev.hip): the assignments of Merkle-membership circuits written by the device, against the host path of the same entry
point (tests/test_merkle_circuit.py pins that one to both host compilers and to the Python builder): at the 64-lane workgroup edges, at depths 1 to 40, with a
padded row stride, over several staged chunks, with non-canonical inputs, and read straight out of a tree's node array."""
import numpy as np
import pytest

import poseidon_util as pu
from openzl_amd import poseidon_merkle_assignment_elems, poseidon_merkle_assignments_host, poseidon_merkle_nodes
from openzl_amd import backend as zb

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
EINVAL = -1
COUNTS = (1, 63, 64, 65, 130)
SENTINEL = 0xA5A5A5A5A5A5A5A5

_REF = {}


def ref(curve, depth):
    """130 memberships with the host path's rows, computed once per (curve, depth) and shared: leaves 0 and r - 1, indices 0 and 2^depth - 1 and a zero
    sibling in the first lanes and in the lanes around the workgroup edge, random elsewhere"""
    if (curve.name, depth) not in _REF:
        r = curve.fr.p
        rng = np.random.default_rng(900 + depth)
        leaves = pu.random_elems(curve, 130, 421 + depth)
        paths = np.array(pu.random_elems(curve, 130 * depth, 422 + depth), dtype=object).reshape(130, depth)
        idx = [int(rng.integers(0, 1 << min(depth, 62))) for _ in range(130)]
        for base in (0, 62, 127):
            leaves[base], leaves[base + 1] = 0, r - 1
            idx[base], idx[base + 1] = 0, (1 << depth) - 1
            paths[base + 2, 0] = 0
            paths[base + 1, depth - 1] = 0
        lv, pa = pu.limbs(leaves), pu.limbs(paths.reshape(-1)).reshape(130, depth, 4)
        ix = np.array(idx, dtype=np.uint64)
        exp = poseidon_merkle_assignments_host(curve.cid, lv, ix, pa, depth)
        exp.setflags(write=False)
        _REF[(curve.name, depth)] = (lv, ix, pa, exp)
    return _REF[(curve.name, depth)]


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
@pytest.mark.parametrize("depth", [1, 2, 5, 40])
def test_device_rows_equal_the_host_path_at_workgroup_edges(backend, curve, depth):
    lv, ix, pa, exp = ref(curve, depth)
    nv = poseidon_merkle_assignment_elems(depth)
    assert nv == 3 + 238 * depth
    for count in COUNTS:
        got = backend.poseidon_merkle_assignments(curve.cid, lv[:count], ix[:count], pa[:count], depth)
        assert got.shape == (count, nv, 4)
        assert got.tobytes() == exp[:count].tobytes(), count
    assert backend.poseidon_merkle_assignments(curve.cid, lv[:0], ix[:0], pa[:0], depth).shape == (0, nv, 4)
    # the roots are the folds of the existing entry point
    assert np.array_equal(exp[:, 1], backend.poseidon_merkle_roots_from_paths(curve.cid, lv, ix, pa, depth))


@CURVES
@pytest.mark.parametrize("depth", [1, 2, 5])
def test_device_pointers_with_a_padded_stride_leave_the_padding_alone(backend, curve, depth):
    lv, ix, pa, exp = ref(curve, depth)
    nv = poseidon_merkle_assignment_elems(depth)
    stride = nv + 5
    d_lv, d_pa = dev(lv), dev(pa)
    for count in COUNTS:
        d_out = dev(np.full((count + 1, stride, 4), SENTINEL, dtype=np.uint64))  # one spare row behind the batch
        backend.poseidon_merkle_assignments_dev(curve.cid, d_lv.data_ptr(), ix[:count], d_pa.data_ptr(), depth, d_out.data_ptr(), stride)
        out = host(d_out).reshape(count + 1, stride, 4)
        assert out[:count, :nv].tobytes() == exp[:count].tobytes(), count
        assert (out[:count, nv:] == SENTINEL).all() and (out[count] == SENTINEL).all(), count
    d_out = dev(np.full((130, nv, 4), SENTINEL, dtype=np.uint64))
    backend.poseidon_merkle_assignments_dev(curve.cid, d_lv.data_ptr(), ix, d_pa.data_ptr(), depth, d_out.data_ptr())  # default: dense rows
    assert host(d_out).tobytes() == exp.tobytes()
    backend.poseidon_merkle_assignments_dev(curve.cid, d_lv.data_ptr(), ix[:0], d_pa.data_ptr(), depth, d_out.data_ptr())
    bad_ix = ix[:2].copy()
    bad_ix[1] = 1 << depth
    for bad_stride, ptr, idx in ((nv - 1, d_out.data_ptr(), ix[:2]), (nv, d_out.data_ptr() + 8, ix[:2]), (nv, d_out.data_ptr(), bad_ix)):
        with pytest.raises(zb.BackendError) as e:  # a stride below the row, a destination off 16 bytes, an index at 2^depth
            backend.poseidon_merkle_assignments_dev(curve.cid, d_lv.data_ptr(), idx, d_pa.data_ptr(), depth, ptr, bad_stride)
        assert e.value.code == EINVAL


@CURVES
def test_three_staged_chunks(backend, curve, device_path):
    device_path.setenv("ZL_TUNE_POSEIDON_CHUNK", "48")  # 48 + 48 + 34 memberships
    lv, ix, pa, exp = ref(curve, 2)
    assert backend.poseidon_merkle_assignments(curve.cid, lv, ix, pa, 2).tobytes() == exp.tobytes()
    d_lv, d_pa, d_out = dev(lv), dev(pa), dev(np.zeros((130, 479, 4), dtype=np.uint64))
    backend.poseidon_merkle_assignments_dev(curve.cid, d_lv.data_ptr(), ix, d_pa.data_ptr(), 2, d_out.data_ptr())
    assert host(d_out).tobytes() == exp.tobytes()


@CURVES
def test_non_canonical_leaf_or_sibling_is_refused_and_the_ctx_lives_on(backend, curve, device_path):
    lv, ix, pa, exp = ref(curve, 2)
    for which, value in (("leaf", curve.fr.p), ("sibling", curve.fr.p), ("sibling", (1 << 256) - 1)):
        bad_lv, bad_pa = lv.copy(), pa.copy()
        if which == "leaf":
            bad_lv[70] = pu.limbs([value])[0]
        else:
            bad_pa[70, 1] = pu.limbs([value])[0]
        with pytest.raises(zb.BackendError) as e:
            backend.poseidon_merkle_assignments(curve.cid, bad_lv, ix, bad_pa, 2)
        assert e.value.code == EINVAL
        d_lv, d_pa, d_out = dev(bad_lv), dev(bad_pa), dev(np.zeros((130, 479, 4), dtype=np.uint64))
        with pytest.raises(zb.BackendError) as e:
            backend.poseidon_merkle_assignments_dev(curve.cid, d_lv.data_ptr(), ix, d_pa.data_ptr(), 2, d_out.data_ptr())
        assert e.value.code == EINVAL
    device_path.setenv("ZL_TUNE_POSEIDON_CHUNK", "48")  # ... in the second of three chunks
    with pytest.raises(zb.BackendError) as e:
        backend.poseidon_merkle_assignments(curve.cid, bad_lv, ix, bad_pa, 2)
    assert e.value.code == EINVAL
    assert backend.poseidon_merkle_assignments(curve.cid, lv, ix, pa, 2).tobytes() == exp.tobytes()  # the flag does not stick


@CURVES
@pytest.mark.parametrize("n,depth", [(1, 1), (5, 3), (8, 3), (100, 7)])
def test_memberships_out_of_a_device_tree(backend, curve, n, depth):
    """the member form reads leaf and siblings out of the node array: its rows are the paths form's over the gathered paths, and every root is the tree's"""
    leaves = pu.random_elems(curve, n, 500 + n)
    leaves[0] = 0
    leaves[n - 1] = curve.fr.p - 1 if n > 1 else leaves[n - 1]
    lv = pu.limbs(leaves)
    d_nodes = dev(np.zeros((poseidon_merkle_nodes(n, depth), 4), dtype=np.uint64))
    d_lv = dev(lv)
    root = backend.poseidon_merkle_build_dev(curve.cid, d_lv.data_ptr(), n, depth, d_nodes.data_ptr())
    ix = np.arange(n, dtype=np.uint64)[::-1].copy()  # every leaf, in an order that is not the array's
    paths = backend.poseidon_merkle_paths(curve.cid, d_nodes.data_ptr(), n, depth, ix)
    exp = backend.poseidon_merkle_assignments(curve.cid, lv[ix.astype(np.int64)], ix, paths, depth)
    nv = poseidon_merkle_assignment_elems(depth)
    stride = nv + 5
    d_out = dev(np.full((n + 1, stride, 4), SENTINEL, dtype=np.uint64))
    backend.poseidon_merkle_member_assignments_dev(curve.cid, d_nodes.data_ptr(), n, depth, ix, d_out.data_ptr(), stride)
    out = host(d_out).reshape(n + 1, stride, 4)
    assert out[:n, :nv].tobytes() == exp.tobytes()
    assert (out[:n, nv:] == SENTINEL).all() and (out[n] == SENTINEL).all()
    assert np.array_equal(out[:n, 1], np.tile(root, (n, 1)))
    if n % 2 == 1:
        assert not out[0, 3].any()  # row 0 is the last leaf: in a tree with an odd leaf count its sibling is absent, the zero digest
    for bad in (n, 1 << depth):
        with pytest.raises(zb.BackendError) as e:
            backend.poseidon_merkle_member_assignments_dev(curve.cid, d_nodes.data_ptr(), n, depth, np.array([0, bad], dtype=np.uint64), d_out.data_ptr(), stride)
        assert e.value.code == EINVAL
    with pytest.raises(zb.BackendError) as e:  # more leaves than the depth holds
        backend.poseidon_merkle_member_assignments_dev(curve.cid, d_nodes.data_ptr(), (1 << depth) + 1, depth, ix[:1], d_out.data_ptr(), stride)
    assert e.value.code == EINVAL
