"""Batched Poseidon on the device (csrc/zl_poseidon_dev.hip): permutations, hashes, chains, Merkle builds (wide levels and the one-workgroup tail), path
gathers and path folds against the Python model of tests/poseidon_util.py, the reference fixture and the host path, at the smallest shapes that reach each
branch: wave and block boundaries, several chunks, every tail threshold, absent siblings, forked lanes, a foreign stream."""
import json
import os

import numpy as np
import pytest

import oracle_lib as ol
import poseidon_util as pu
from oracle_lib import po
from openzl_amd import Circuit, Groth16Keys
from openzl_amd import backend as zb

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FX = json.load(open(os.path.join(HERE, "golden", "ref_poseidon_fixtures.json")))
CURVES = pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
EINVAL = -1
HUGE = str(1 << 30)


@pytest.fixture(autouse=True)
def device_path(monkeypatch):
    """every host-pointer call of this file runs on the device unless a test says otherwise"""
    monkeypatch.setenv("ZL_TUNE_POSEIDON_DEV_MIN", "0")


_REF = {}


def ref_hashes(curve):
    """257 + 9 states (random, then 0 / 1 / r - 1 in every position) with their permutations, computed once per curve and shared"""
    if curve.name not in _REF:
        r = curve.fr.p
        vals = pu.random_elems(curve, 3 * 257, 101)
        states = [vals[3 * i:3 * i + 3] for i in range(257)]
        for pos in range(3):
            for v in (0, 1, r - 1):
                st = [3, 7, 11]
                st[pos] = v
                states.append(st)
        _REF[curve.name] = (states, [pu.permute(curve, [3, s[1], s[2]]) for s in states], [pu.permute(curve, s) for s in states])
    return _REF[curve.name]


def dev(a: np.ndarray):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def host(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


# ---- permute / hash2 -----------------------------------------------------------------------------------------------------------------------------------
@CURVES
def test_permute_and_hash2_at_wave_and_block_boundaries(backend, curve):
    states, exp_h, exp_p = ref_hashes(curve)
    edge = list(range(257, 266))
    for count in (1, 63, 64, 65, 255, 256, 257):
        sel = (edge + list(range(257)))[:count] if count >= 9 else list(range(count))
        got = backend.poseidon_permute_batch(curve.cid, pu.limbs([v for i in sel for v in states[i]]))
        assert [pu.ints(g) for g in got] == [exp_p[i] for i in sel], count
        got = backend.poseidon_hash2(curve.cid, pu.limbs([v for i in sel for v in states[i][1:]]))
        assert pu.ints(got) == [exp_h[i][0] for i in sel], count
    assert backend.poseidon_hash2(curve.cid, np.zeros((0, 2, 4), dtype=np.uint64)).shape == (0, 4)


@CURVES
def test_five_chunks_the_last_with_one_element(backend, curve, monkeypatch):
    monkeypatch.setenv("ZL_TUNE_POSEIDON_CHUNK", "256")
    states, exp_h, exp_p = ref_hashes(curve)
    sel = [i % 266 for i in range(1025)]
    got = backend.poseidon_permute_batch(curve.cid, pu.limbs([v for i in sel for v in states[i]]))
    assert [pu.ints(g) for g in got] == [exp_p[i] for i in sel]
    xy = pu.limbs([v for i in sel for v in states[i][1:]])
    got = backend.poseidon_hash2(curve.cid, xy)
    assert pu.ints(got) == [exp_h[i][0] for i in sel]
    d_xy, d_out = dev(xy), dev(np.zeros((1025, 4), dtype=np.uint64))
    backend.poseidon_hash2_dev(curve.cid, d_xy.data_ptr(), 1025, d_out.data_ptr())
    assert np.array_equal(host(d_out).reshape(-1, 4), got)


def test_h_1_2_is_the_reference_digest(backend):
    got = backend.poseidon_hash2(po.BLS12_381.cid, pu.limbs([1, 2]))
    assert str(pu.ints(got)[0]) == FX["permutation_width3"]["output"][0]
    st = backend.poseidon_permute_batch(po.BLS12_381.cid, pu.limbs([3, 1, 2]))
    assert [str(v) for v in pu.ints(st[0])] == FX["permutation_width3"]["output"]


@CURVES
def test_device_buffers_and_host_path_agree_byte_for_byte(backend, curve, monkeypatch):
    states, exp_h, _ = ref_hashes(curve)
    sel = [i % 266 for i in range(300)]
    xy = pu.limbs([v for i in sel for v in states[i][1:]])
    on_dev = backend.poseidon_hash2(curve.cid, xy)
    d_xy, d_out = dev(xy), dev(np.zeros((300, 4), dtype=np.uint64))
    backend.poseidon_hash2_dev(curve.cid, d_xy.data_ptr(), 300, d_out.data_ptr())
    assert np.array_equal(host(d_out).reshape(-1, 4), on_dev)
    monkeypatch.setenv("ZL_TUNE_POSEIDON_DEV_MIN", HUGE)
    on_host = backend.poseidon_hash2(curve.cid, xy)
    assert on_host.tobytes() == on_dev.tobytes()
    assert pu.ints(on_dev) == [exp_h[i][0] for i in sel]


@CURVES
def test_non_canonical_input_is_refused(backend, curve, monkeypatch):
    r = curve.fr.p
    base = pu.random_elems(curve, 3 * 65, 7)
    for at in (0, 3 * 65 - 1):
        vals = list(base)
        vals[at] = r
        with pytest.raises(zb.BackendError) as e:
            backend.poseidon_permute_batch(curve.cid, pu.limbs(vals))
        assert e.value.code == EINVAL
    for at in (0, 2 * 65 - 1):
        vals = list(base[:130])
        vals[at] = r
        with pytest.raises(zb.BackendError) as e:
            backend.poseidon_hash2(curve.cid, pu.limbs(vals))
        assert e.value.code == EINVAL
        d_xy, d_out = dev(pu.limbs(vals)), dev(np.zeros((65, 4), dtype=np.uint64))
        with pytest.raises(zb.BackendError) as e:
            backend.poseidon_hash2_dev(curve.cid, d_xy.data_ptr(), 65, d_out.data_ptr())
        assert e.value.code == EINVAL
    # in the second chunk of a chunked batch
    monkeypatch.setenv("ZL_TUNE_POSEIDON_CHUNK", "32")
    vals = list(base[:130])
    vals[2 * 40 + 1] = (1 << 256) - 1
    with pytest.raises(zb.BackendError) as e:
        backend.poseidon_hash2(curve.cid, pu.limbs(vals))
    assert e.value.code == EINVAL
    assert backend.poseidon_hash2(curve.cid, pu.limbs(base[:130])).shape == (65, 4)  # the flag does not stick


# ---- chain ---------------------------------------------------------------------------------------------------------------------------------------------
@CURVES
def test_chains(backend, curve):
    x0, x1 = pu.random_elems(curve, 65, 201), pu.random_elems(curve, 65, 202)
    x0[:3], x1[:3] = [0, 1, curve.fr.p - 1], [curve.fr.p - 1, 0, 1]
    h = list(x0)
    done = 0
    for k in (1, 2, 8):  # the model walks all 65 chains once up to k = 8 ...
        for _ in range(k - done):
            h = [pu.hash2(curve, a, b) for a, b in zip(h, x1)]
        done = k
        for count in (1, 65):
            got = backend.poseidon_chain(curve.cid, pu.limbs(x0[:count]), pu.limbs(x1[:count]), k)
            assert pu.ints(got) == h[:count], (k, count)
    # ... and the first 13 on to k = 64 (the model's hashes stay near a thousand): lane i of the 65 runs chain i mod 13
    h = h[:13]
    for _ in range(64 - 8):
        h = [pu.hash2(curve, a, b) for a, b in zip(h, x1)]
    lanes = [i % 13 for i in range(65)]
    for count in (1, 65):
        got = backend.poseidon_chain(curve.cid, pu.limbs([x0[i] for i in lanes[:count]]), pu.limbs([x1[i] for i in lanes[:count]]), 64)
        assert pu.ints(got) == [h[i] for i in lanes[:count]], count
    with pytest.raises(zb.BackendError):
        backend.poseidon_chain(curve.cid, pu.limbs(x0[:2]), pu.limbs(x1[:2]), 0)


# ---- Merkle --------------------------------------------------------------------------------------------------------------------------------------------
_TREES = {}


def ref_tree(curve, n, depth):
    """levels of the tree over the first n shared leaves, computed once; the trees above 1 000 leaves through the host zl_poseidon_permute loop
    (tests/test_host_mirror.py pins it to the oracle), the others through the Python model"""
    key = (curve.name, n, depth)
    if key not in _TREES:
        leaves = ref_leaves(curve)[:n]
        _TREES[key] = pu.merkle_levels(curve, leaves, depth, pu.host_loop_hash_fn(curve) if n > 1000 else None)
    return _TREES[key]


def ref_leaves(curve):
    if ("leaves", curve.name) not in _TREES:
        _TREES[("leaves", curve.name)] = pu.random_elems(curve, 4097, 301)
    return _TREES[("leaves", curve.name)]


# 4 097 leaves take depth 13: n <= 2^depth is the rule of the header (4 097 at depth 12 is refused: test_merkle_build_whole_node_array checks that too)
MERKLE_CASES = [(n, 10) for n in (0, 1, 2, 3, 5, 64, 65, 127, 128, 129, 1000, 1024)] + [(4097, 13)]


@CURVES
@pytest.mark.parametrize("tail", ["0", "1", "4", None], ids=lambda t: "tail-" + (t or "default"))
def test_merkle_build_whole_node_array(backend, curve, tail, monkeypatch):
    if tail is None:
        monkeypatch.delenv("ZL_TUNE_POSEIDON_TAIL", raising=False)
    else:
        monkeypatch.setenv("ZL_TUNE_POSEIDON_TAIL", tail)
    assert zb.poseidon_merkle_nodes(4097, 12) == 0
    with pytest.raises(zb.BackendError) as e:
        backend.poseidon_merkle_root(curve.cid, pu.limbs(ref_leaves(curve)), 12)
    assert e.value.code == EINVAL
    for n, depth in MERKLE_CASES:
        lv = ref_tree(curve, n, depth)
        flat = pu.limbs(pu.merkle_flat(lv))
        total = zb.poseidon_merkle_nodes(n, depth)
        assert total == flat.shape[0]
        leaves = pu.limbs(ref_leaves(curve)[:n])
        d_leaves, d_nodes = dev(leaves if n else np.zeros((1, 4), dtype=np.uint64)), dev(np.full((max(1, total), 4), 0xA5A5A5A5, dtype=np.uint64))
        root = backend.poseidon_merkle_build_dev(curve.cid, d_leaves.data_ptr(), n, depth, d_nodes.data_ptr())
        assert pu.ints(root) == [pu.merkle_root(lv)], (n, depth)
        if n:
            assert np.array_equal(host(d_nodes).reshape(-1, 4), flat), (n, depth)
        nodes, root2 = backend.poseidon_merkle_build(curve.cid, leaves, depth)
        assert np.array_equal(nodes, flat) and np.array_equal(root2, root), (n, depth)
        assert np.array_equal(backend.poseidon_merkle_root(curve.cid, leaves, depth), root), (n, depth)


@CURVES
@pytest.mark.parametrize("tail", ["0", None], ids=["tail-0", "tail-default"])
def test_depth_beyond_the_leaves(backend, curve, tail, monkeypatch):
    """n = 3 at depth 10: two real levels, then eight H(., 0)"""
    if tail is not None:
        monkeypatch.setenv("ZL_TUNE_POSEIDON_TAIL", tail)
    lv = ref_tree(curve, 3, 10)
    exp = pu.hash2(curve, pu.hash2(curve, lv[0][0], lv[0][1]), pu.hash2(curve, lv[0][2], 0))
    for _ in range(8):
        exp = pu.hash2(curve, exp, 0)
    assert pu.ints(backend.poseidon_merkle_root(curve.cid, pu.limbs(lv[0]), 10)) == [exp] == [pu.merkle_root(lv)]


@CURVES
def test_non_canonical_leaf_is_refused_on_both_build_paths(backend, curve, monkeypatch):
    leaves = pu.limbs(ref_leaves(curve)[:129] + [curve.fr.p])
    for tail in ("0", "256"):
        monkeypatch.setenv("ZL_TUNE_POSEIDON_TAIL", tail)
        with pytest.raises(zb.BackendError) as e:
            backend.poseidon_merkle_root(curve.cid, leaves, 10)
        assert e.value.code == EINVAL


@CURVES
def test_paths_and_folds(backend, curve, monkeypatch):
    n, depth = 129, 10
    lv = ref_tree(curve, n, depth)
    root = pu.merkle_root(lv)
    leaves = ref_leaves(curve)[:n]
    d_nodes = dev(pu.limbs(pu.merkle_flat(lv)))
    idx = list(range(n)) + [128, 0, 0, 77]  # every index, then duplicates
    paths = backend.poseidon_merkle_paths(curve.cid, d_nodes.data_ptr(), n, depth, idx)
    assert [pu.ints(p) for p in paths] == [pu.merkle_path(lv, i) for i in idx]
    assert pu.merkle_path(lv, 128)[:7] == [0] * 7  # (absent siblings at several levels are in the case)
    for count in (1, 64, 129):
        sel = idx[n - count:n] if count < n else idx[:n]
        got = backend.poseidon_merkle_roots_from_paths(curve.cid, pu.limbs([leaves[i] for i in sel]), sel, paths[sel], depth)
        assert pu.ints(got) == [root] * count, count
    bad = paths[:n].copy()
    bad[5, 3, 1] ^= np.uint64(1)
    bad[128, 0, 0] ^= np.uint64(1)  # an absent (zero) sibling replaced
    got = pu.ints(backend.poseidon_merkle_roots_from_paths(curve.cid, pu.limbs(leaves), idx[:n], bad, depth))
    assert [g == root for g in got] == [i not in (5, 128) for i in range(n)]
    wrong = [i ^ (1 << (i % depth)) for i in range(n)]
    got = pu.ints(backend.poseidon_merkle_roots_from_paths(curve.cid, pu.limbs(leaves), wrong, paths[:n], depth))
    assert all(g != root for g in got)
    assert got[:4] == [pu.fold_path(curve, leaves[i], wrong[i], pu.merkle_path(lv, i)) for i in range(4)]
    with pytest.raises(zb.BackendError) as e:
        backend.poseidon_merkle_paths(curve.cid, d_nodes.data_ptr(), n, depth, [0, n])
    assert e.value.code == EINVAL
    # several staged chunks
    monkeypatch.setenv("ZL_TUNE_POSEIDON_CHUNK", "50")
    assert np.array_equal(backend.poseidon_merkle_paths(curve.cid, d_nodes.data_ptr(), n, depth, idx), paths)
    got = backend.poseidon_merkle_roots_from_paths(curve.cid, pu.limbs(leaves), idx[:n], paths[:n], depth)
    assert pu.ints(got) == [root] * n


# ---- lanes and streams ---------------------------------------------------------------------------------------------------------------------------------
@CURVES
def test_forked_lane_and_foreign_stream(backend, curve):
    import torch

    states, exp_h, _ = ref_hashes(curve)
    xy = pu.limbs([v for s in states[:130] for v in s[1:]])
    exp = [h[0] for h in exp_h[:130]]
    lv = ref_tree(curve, 129, 10)
    leaves = pu.limbs(lv[0])
    lane = backend.fork()
    try:
        assert pu.ints(lane.poseidon_hash2(curve.cid, xy)) == exp
        nodes, root = lane.poseidon_merkle_build(curve.cid, leaves, 10)
        assert pu.ints(nodes) == pu.merkle_flat(lv) and pu.ints(root) == [pu.merkle_root(lv)]
    finally:
        lane.close()
        backend._forks.remove(lane)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        backend.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            d_xy = torch.from_numpy(xy.view(np.int64).copy()).cuda(non_blocking=False)
            d_out = torch.zeros(130 * 4, dtype=torch.int64, device="cuda")
            backend.poseidon_hash2_dev(curve.cid, d_xy.data_ptr(), 130, d_out.data_ptr())
            assert pu.ints(host(d_out)) == exp
            assert pu.ints(backend.poseidon_merkle_root(curve.cid, leaves, 10)) == [pu.merkle_root(lv)]
        finally:
            backend.set_stream(0)


# ---- integration ---------------------------------------------------------------------------------------------------------------------------------------
def test_chain_outputs_are_the_public_inputs_batch_verification_accepts(backend):
    curve = po.BLS12_381
    x0s, x1 = [11, 12, 13], 2
    circuits = [Circuit(curve.cid, 1, x0, x1) for x0 in x0s]
    keys = Groth16Keys(backend, circuits[0], seed=0x905E1D)
    try:
        proofs = [keys.prove(seed=500 + i, circuit=c)[0] for i, c in enumerate(circuits)]
        pubs = backend.poseidon_chain(curve.cid, pu.limbs(x0s), pu.limbs([x1] * 3), 1)
        assert np.array_equal(pubs, np.stack([c.arrays()["assignment"][1] for c in circuits]))
        ok, each = keys.verify_batch(proofs, pubs.reshape(3, 1, 4), seed=5, each=True)
        assert ok and each.all()
        altered = backend.poseidon_chain(curve.cid, pu.limbs([11, 12, 14]), pu.limbs([x1] * 3), 1)
        ok, each = keys.verify_batch(proofs, altered.reshape(3, 1, 4), seed=5, each=True)
        assert not ok and list(each) == [True, True, False]
    finally:
        keys.close()
        for c in circuits:
            c.close()
