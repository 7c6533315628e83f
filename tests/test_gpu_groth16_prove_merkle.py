"""zl_groth16_prove_merkle_paths / _members: memberships in, proofs out -- k_pos_merkle_trace writes the assignments straight into the batch's block.  Every
proof must equal zl_groth16_prove_resident for the same (assignment, r, s) byte for byte, on the device path (forced with ZL_TUNE_G16_BATCH_LOG_N / _MIN) and on
both fallbacks to the loop over the resident prover; one proof per curve also equals the C oracle's over the Python builder's matrices, which puts a circuit of
Boolean and select rows against the oracle end to end; and a tree built on the device is proven and batch-verified with default dispatch."""
import numpy as np
import pytest

import groth16_util as gu
import merkle_circuit_util as mu
import oracle_lib as ol
import poseidon_util as pu
from openzl_amd import BackendError, Circuit, Groth16Keys, poseidon_merkle_assignments_host, poseidon_merkle_nodes

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
EINVAL, EHANDLE = -1, -5


def _same(p, q):
    return all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(p, q))


def dev(a: np.ndarray):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


@pytest.fixture
def device_path(monkeypatch):
    monkeypatch.setenv("ZL_TUNE_G16_BATCH_LOG_N", "28")
    monkeypatch.setenv("ZL_TUNE_G16_BATCH_MIN", "1")
    monkeypatch.setenv("ZL_TUNE_POSEIDON_DEV_MIN", "0")
    return monkeypatch


def _rs(curve, count, seed):
    """distinct blinding scalars with one r and one s zero"""
    rs = ol.random_scalars(curve, 2 * count, seed)
    r, s = np.ascontiguousarray(rs[:count]), np.ascontiguousarray(rs[count:])
    r[min(3, count - 1)] = 0
    s[min(4, count - 1)] = 0
    return r, s


def _make(backend, curve, depth, count, seed):
    """keys of the depth-`depth` membership circuit, `count` memberships (leaf 0, leaf r - 1, a zero sibling, indices 0 and 2^depth - 1 among them) with the
    host path's assignments (tests/test_merkle_circuit.py pins them to the compilers'), blinding scalars, and the resident prover's proof of each"""
    p = curve.fr.p
    leaves = pu.random_elems(curve, count, seed + 2)
    paths = [pu.random_elems(curve, depth, seed + 3 + j) for j in range(count)]
    idx = [(5 * j + 1) % (1 << depth) for j in range(count)]
    leaves[0], idx[0] = 0, 0
    if count > 2:
        leaves[1], idx[1] = p - 1, (1 << depth) - 1
        paths[2][0] = 0
    full = Circuit.merkle(curve.cid, depth, leaves[0], idx[0], paths[0])
    keys = Groth16Keys(backend, full, seed=seed)
    lv, ix = pu.limbs(leaves), np.array(idx, dtype=np.uint64)
    pa = pu.limbs([v for row in paths for v in row]).reshape(count, depth, 4)
    Z = poseidon_merkle_assignments_host(curve.cid, lv, ix, pa, depth)
    r, s = _rs(curve, count, seed + 1)
    hr = backend.r1cs_upload(curve.cid, full.arrays())
    pk = keys.pk_dict()
    ref = [backend.groth16_prove_resident(curve.cid, pk, hr, Z[j], r[j], s[j]) for j in range(count)]
    return dict(full=full, keys=keys, leaves=leaves, idx=idx, paths=paths, lv=lv, ix=ix, pa=pa, Z=Z, r=r, s=s, hr=hr, pk=pk, ref=ref, depth=depth)


def _drop(backend, made):
    for m in made.values():
        backend.r1cs_free(m["hr"])
        m["keys"].close()
        m["full"].close()


def _shared(backend, depth, count, seed):
    made = {}

    def get(curve):
        if curve.cid not in made:
            made[curve.cid] = _make(backend, curve, depth, count, seed)
        return made[curve.cid]

    return made, get


@pytest.fixture(scope="module")
def depth1(backend):
    """per curve: the depth-1 circuit (domain 2^8) with 130 proofs' worth of references, computed once and shared"""
    made, get = _shared(backend, 1, 130, 1771)
    yield get
    _drop(backend, made)


@pytest.fixture(scope="module")
def depth2(backend):
    """per curve: the depth-2 circuit (domain 2^9) with 7 references"""
    made, get = _shared(backend, 2, 7, 1881)
    yield get
    _drop(backend, made)


def _check(m, got, count):
    return len(got) == count and all(_same(got[j], m["ref"][j]) for j in range(count))


def _domain(m):
    return 1 << max(1, (m["full"].shape[0] + m["full"].shape[1] - 1).bit_length())


def _fallbacks(m):
    """the two settings that send a batch of 7 to the loop over the resident prover"""
    yield {"ZL_TUNE_G16_BATCH_LOG_N": str(_domain(m).bit_length() - 2), "ZL_TUNE_G16_BATCH_MIN": "1"}  # the domain bound below the circuit
    yield {"ZL_TUNE_G16_BATCH_LOG_N": "28", "ZL_TUNE_G16_BATCH_MIN": "8"}                              # the minimum count above the batch


def _paths(m, count):
    return m["lv"][:count], m["ix"][:count], m["pa"][:count], m["r"][:count], m["s"][:count]


@CURVES
@pytest.mark.parametrize("count", [1, 7, 130])
def test_prove_paths_equals_resident_and_verifies(backend, depth1, device_path, curve, count):
    m = depth1(curve)
    assert _domain(m) == 1 << 8 and m["keys"].merkle_depth() == 1 and m["keys"].chain_links() == 0
    got, roots = m["keys"].prove_merkle_paths(*_paths(m, count))
    assert _check(m, got, count)
    assert np.array_equal(roots, m["Z"][:count, 1])
    assert pu.ints(roots) == [mu.fold(curve, m["leaves"][j], m["idx"][j], m["paths"][j]) for j in range(count)]
    assert m["keys"].verify_batch(got, roots.reshape(count, 1, 4))
    with pytest.raises(BackendError) as e:
        backend.groth16_last_h(2)  # the device path ran: no single quotient
    assert e.value.code == EINVAL


@CURVES
def test_prove_paths_depth_two_chunks_lane_and_fallbacks(backend, depth2, device_path, curve):
    m = depth2(curve)
    count = 7
    args = _paths(m, count)
    exp_roots = m["Z"][:count, 1]
    assert _domain(m) == 1 << 9 and m["keys"].merkle_depth() == 2
    got, roots = m["keys"].prove_merkle_paths(*args)
    assert _check(m, got, count) and np.array_equal(roots, exp_roots)
    device_path.setenv("ZL_TUNE_G16_BATCH_CHUNK", "3")   # 3 + 3 + 1 proofs ...
    device_path.setenv("ZL_TUNE_POSEIDON_CHUNK", "2")    # ... whose traces run as 2 + 1, 2 + 1 and 1
    got, roots = m["keys"].prove_merkle_paths(*args)
    assert _check(m, got, count) and np.array_equal(roots, exp_roots)
    assert m["keys"].verify_batch(got, roots.reshape(count, 1, 4))
    device_path.delenv("ZL_TUNE_G16_BATCH_CHUNK")
    device_path.delenv("ZL_TUNE_POSEIDON_CHUNK")
    lane = backend.fork()
    try:
        got, roots = m["keys"].prove_merkle_paths(*args, lane=lane)
        assert _check(m, got, count) and np.array_equal(roots, exp_roots)
    finally:
        lane.close()
        backend._forks.remove(lane)
    n = _domain(m)
    for env in _fallbacks(m):
        for key, v in env.items():
            device_path.setenv(key, v)
        for dev_min in ("0", str(1 << 30)):  # the assignments of the fallback from the device, and from the host mirror
            device_path.setenv("ZL_TUNE_POSEIDON_DEV_MIN", dev_min)
            got, roots = m["keys"].prove_merkle_paths(*args)
            assert _check(m, got, count) and np.array_equal(roots, exp_roots)
            assert backend.groth16_last_h(n).shape == (n, 4)  # the resident prover ran and left its quotient


@CURVES
def test_prove_paths_depth_one_chunks_and_fallbacks(backend, depth1, device_path, curve):
    m = depth1(curve)
    count = 7
    args = _paths(m, count)
    device_path.setenv("ZL_TUNE_G16_BATCH_CHUNK", "3")
    got, roots = m["keys"].prove_merkle_paths(*args)
    assert _check(m, got, count) and np.array_equal(roots, m["Z"][:count, 1])
    device_path.delenv("ZL_TUNE_G16_BATCH_CHUNK")
    n = _domain(m)
    for env in _fallbacks(m):
        for key, v in env.items():
            device_path.setenv(key, v)
        got, roots = m["keys"].prove_merkle_paths(*args)
        assert _check(m, got, count) and np.array_equal(roots, m["Z"][:count, 1])
        assert backend.groth16_last_h(n).shape == (n, 4)


@CURVES
def test_proof_and_quotient_equal_the_oracle_on_the_python_builders_matrices(backend, depth2, device_path, curve):
    """Boolean and select rows against the C oracle end to end: its matrices are the Python builder's, its key the queries the library's setup made"""
    m = depth2(curve)
    j = 2  # the membership with a zero sibling
    cs = mu.poseidon_merkle_circuit(curve.fr, 2, m["leaves"][j], m["idx"][j], m["paths"][j])
    assert cs.is_satisfied()
    z = ol.ints_to_limbs(cs.assignment(), 4)
    assert np.array_equal(z, m["Z"][j])
    pk = dict(m["pk"])
    for name in ("a_query", "b_g1_query", "h_query", "l_query", "b_g2_query"):
        pk[name] = backend.bases_download(m["pk"][name])
    n = _domain(m)
    exp, h = gu.oracle_prove(curve, gu.r1cs_arrays(cs), z, pk, m["r"][j], m["s"][j], threads=8, want_h=n)
    sl = slice(j, j + 1)
    got, roots = m["keys"].prove_merkle_paths(m["lv"][sl], m["ix"][sl], m["pa"][sl], m["r"][sl], m["s"][sl])  # the device path
    assert _same(got[0], exp) and np.array_equal(roots[0], z[1])
    device_path.setenv("ZL_TUNE_G16_BATCH_MIN", "8")  # the resident loop: it leaves its quotient
    got, roots = m["keys"].prove_merkle_paths(m["lv"][sl], m["ix"][sl], m["pa"][sl], m["r"][sl], m["s"][sl])
    assert _same(got[0], exp)
    assert np.array_equal(backend.groth16_last_h(n), h)


@CURVES
def test_errors(backend, depth1, device_path, curve):
    m = depth1(curve)
    lv, ix, pa, r, s = _paths(m, 4)
    pk, hr = m["pk"], m["hr"]
    chain = Circuit(curve.cid, 1)
    chain_keys = Groth16Keys(backend, chain, seed=5)
    try:
        assert chain_keys.merkle_depth() == 0
        with pytest.raises(ValueError):  # keys of a chain circuit are refused ...
            chain_keys.prove_merkle_paths(lv, ix, pa, r, s)
        with pytest.raises(ValueError):
            chain_keys.prove_merkle_members(0, 1, ix[:0], r[:0], s[:0])
        hc = backend.r1cs_upload(curve.cid, chain.arrays())
        try:
            with pytest.raises(BackendError) as e:  # ... by the library too
                backend.groth16_prove_merkle_paths(curve.cid, chain_keys.pk_dict(), hc, 1, lv, ix, pa, r, s)
            assert e.value.code == EINVAL
            with pytest.raises(BackendError) as e:  # and the chain prover refuses a membership circuit
                backend.groth16_prove_poseidon_chains(curve.cid, pk, hr, 1, lv, lv, r, s)
            assert e.value.code == EINVAL
        finally:
            backend.r1cs_free(hc)
    finally:
        chain_keys.close()
        chain.close()
    pa2 = np.ascontiguousarray(np.concatenate([pa, pa], axis=1))
    for log_n in ("28", "0"):  # on the device path and on the fallback
        device_path.setenv("ZL_TUNE_G16_BATCH_LOG_N", log_n)
        pa41 = np.ascontiguousarray(np.tile(pa, (1, 41, 1)))
        for depth, paths in ((2, pa2), (0, pa), (41, pa41)):  # a depth that is not the circuit's, and depths outside 1..40
            with pytest.raises(BackendError) as e:
                backend.groth16_prove_merkle_paths(curve.cid, pk, hr, depth, lv, ix, paths, r, s)
            assert e.value.code == EINVAL
        with pytest.raises(BackendError) as e:
            backend.groth16_prove_merkle_paths(curve.cid, pk, 0x7FFF0001, 1, lv, ix, pa, r, s)
        assert e.value.code == EHANDLE
        bad_ix = ix.copy()
        bad_ix[2] = 2  # == 2^depth
        with pytest.raises(BackendError) as e:
            m["keys"].prove_merkle_paths(lv, bad_ix, pa, r, s)
        assert e.value.code == EINVAL
        for which in ("leaf", "sibling"):
            bad_lv, bad_pa = lv.copy(), pa.copy()
            if which == "leaf":
                bad_lv[2] = pu.limbs([curve.fr.p])[0]
            else:
                bad_pa[2, 0] = pu.limbs([curve.fr.p])[0]
            with pytest.raises(BackendError) as e:
                m["keys"].prove_merkle_paths(bad_lv, ix, bad_pa, r, s)
            assert e.value.code == EINVAL
        got, roots = m["keys"].prove_merkle_paths(lv[:0], ix[:0], pa[:0], r[:0], s[:0])  # count == 0
        assert got == [] and roots.shape == (0, 4)
        got, roots = backend.groth16_prove_merkle_paths(curve.cid, pk, hr, 1, lv, ix, pa, r, s)  # usable after the errors
        assert _check(m, got, 4) and np.array_equal(roots, m["Z"][:4, 1])
        # the member form: a tree of two leaves at depth 1
        d_nodes = dev(np.zeros((poseidon_merkle_nodes(2, 1), 4), dtype=np.uint64))
        backend.poseidon_merkle_build_dev(curve.cid, dev(lv[:2]).data_ptr(), 2, 1, d_nodes.data_ptr())
        for n_leaves, idx in ((2, [0, 2]), (3, [0, 1])):  # an index at n; more leaves than the depth holds
            with pytest.raises(BackendError) as e:
                m["keys"].prove_merkle_members(d_nodes.data_ptr(), n_leaves, idx, r[:2], s[:2])
            assert e.value.code == EINVAL
        got, root = m["keys"].prove_merkle_members(d_nodes.data_ptr(), 2, [], r[:0], s[:0])
        assert got == []


@CURVES
def test_members_on_forced_paths_equal_the_paths_form(backend, depth2, device_path, curve):
    """a 3-leaf tree at depth 2 (absent siblings at both levels): the member form's proofs are the paths form's over the gathered paths, on the device path
    and on the fallback, where the rows the device wrote come back through host staging"""
    m = depth2(curve)
    n, depth = 3, 2
    lv = m["lv"][:n]
    d_nodes = dev(np.zeros((poseidon_merkle_nodes(n, depth), 4), dtype=np.uint64))
    root = backend.poseidon_merkle_build_dev(curve.cid, dev(lv).data_ptr(), n, depth, d_nodes.data_ptr())
    ix = np.array([2, 0, 1, 2, 2], dtype=np.uint64)
    r, s = _rs(curve, ix.size, 99)
    paths = backend.poseidon_merkle_paths(curve.cid, d_nodes.data_ptr(), n, depth, ix)
    exp, roots = m["keys"].prove_merkle_paths(lv[ix.astype(np.int64)], ix, paths, r, s)
    assert np.array_equal(roots, np.tile(root, (ix.size, 1)))
    got, got_root = m["keys"].prove_merkle_members(d_nodes.data_ptr(), n, ix, r, s)
    assert len(got) == ix.size and all(_same(a, b) for a, b in zip(got, exp)) and np.array_equal(got_root, root)
    device_path.setenv("ZL_TUNE_G16_BATCH_CHUNK", "2")
    device_path.setenv("ZL_TUNE_POSEIDON_CHUNK", "1")
    got, got_root = m["keys"].prove_merkle_members(d_nodes.data_ptr(), n, ix, r, s)
    assert all(_same(a, b) for a, b in zip(got, exp)) and np.array_equal(got_root, root)
    device_path.setenv("ZL_TUNE_G16_BATCH_MIN", "8")  # the resident loop
    got, got_root = m["keys"].prove_merkle_members(d_nodes.data_ptr(), n, ix, r, s)
    assert all(_same(a, b) for a, b in zip(got, exp)) and np.array_equal(got_root, root)
    assert backend.groth16_last_h(_domain(m)).shape == (_domain(m), 4)
    assert m["keys"].verify_batch(got, np.tile(root, (ix.size, 1)).reshape(ix.size, 1, 4))


@CURVES
def test_tree_to_proofs_with_default_dispatch(backend, curve, monkeypatch):
    """no tuning variable set: a 100-leaf tree at depth 7 built on the device, 70 memberships proven from the node array.  The domain is 2^11 and 70 >= 64, so
    the batch takes the device path; every proof is the resident prover's for the same row, and the batch verifies against the one root"""
    for name in ("ZL_TUNE_G16_BATCH_LOG_N", "ZL_TUNE_G16_BATCH_MIN", "ZL_TUNE_G16_BATCH_CHUNK", "ZL_TUNE_POSEIDON_DEV_MIN", "ZL_TUNE_POSEIDON_CHUNK",
                 "ZL_TUNE_POSEIDON_TAIL"):
        monkeypatch.delenv(name, raising=False)
    n, depth, count = 100, 7, 70
    leaves = pu.random_elems(curve, n, 6100)
    leaves[0], leaves[99] = 0, curve.fr.p - 1
    lv = pu.limbs(leaves)
    d_nodes = dev(np.zeros((poseidon_merkle_nodes(n, depth), 4), dtype=np.uint64))
    root = backend.poseidon_merkle_build_dev(curve.cid, dev(lv).data_ptr(), n, depth, d_nodes.data_ptr())
    ix = np.array([(37 * j + 99) % n for j in range(count)], dtype=np.uint64)  # 70 distinct leaves, the last one (absent siblings) first
    assert len(set(ix.tolist())) == count and ix[0] == 99
    full = Circuit.merkle(curve.cid, depth, 1, 0, [2] * depth)
    keys = Groth16Keys(backend, full, seed=6101)
    hr = backend.r1cs_upload(curve.cid, full.arrays())
    try:
        assert keys.merkle_depth() == depth and 1 << max(1, (full.shape[0] + full.shape[1] - 1).bit_length()) == 1 << 11
        r, s = _rs(curve, count, 6102)
        got, got_root = keys.prove_merkle_members(d_nodes.data_ptr(), n, ix, r, s)
        assert np.array_equal(got_root, root)
        with pytest.raises(BackendError):
            backend.groth16_last_h(2)  # the device path ran
        d_rows = dev(np.zeros((count, 3 + 238 * depth, 4), dtype=np.uint64))
        backend.poseidon_merkle_member_assignments_dev(curve.cid, d_nodes.data_ptr(), n, depth, ix, d_rows.data_ptr())
        rows = d_rows.cpu().numpy().view(np.uint64).reshape(count, 3 + 238 * depth, 4)
        assert np.array_equal(rows[:, 1], np.tile(root, (count, 1))) and np.array_equal(rows[:, 2], lv[ix.astype(np.int64)])
        pk = keys.pk_dict()
        for j in range(count):
            assert _same(got[j], backend.groth16_prove_resident(curve.cid, pk, hr, rows[j], r[j], s[j])), j
        pubs = np.tile(root, (count, 1)).reshape(count, 1, 4)
        assert keys.verify_batch(got, pubs)
        pubs[5, 0] = lv[5]  # another value as one proof's public input
        assert not keys.verify_batch(got, pubs)
    finally:
        backend.r1cs_free(hr)
        keys.close()
        full.close()
