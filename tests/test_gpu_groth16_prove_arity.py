"""zl_groth16_prove_poseidon_hashes / zl_groth16_prove_merkle_leaf_paths / _members: inputs in, proofs out -- k_pos_hash_trace and k_pos_leaf_merkle_trace write
the assignments of the arity-general circuits straight into the batch's block.  Every proof must equal zl_groth16_prove_resident for the same (host-mirror row,
r, s) byte for byte, on the device path (forced with ZL_TUNE_G16_BATCH_LOG_N / _MIN) and on both fallbacks to the loop over the resident prover; one proof per
curve and circuit also equals the C oracle's over the Python builder's matrices; keys of another shape are refused; and a tree built on the device from its
leaves' preimages is proven and batch-verified against the root the call returns."""
import numpy as np
import pytest

import arity_circuit_util as au
import groth16_util as gu
import oracle_lib as ol
import poseidon_arity_util as pa
import poseidon_util as pu
from openzl_amd import (BackendError, Circuit, Groth16Keys, poseidon_hash_assignments_host, poseidon_merkle_leaf_assignments_host, poseidon_merkle_nodes)

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
EINVAL, EHANDLE = -1, -5
# (arity, proofs): the first shape of each family runs 130 proofs over several chunks, the other 7
HASH_SHAPES = [(3, 130), (5, 7)]
# (arity, depth, proofs)
LEAF_SHAPES = [(4, 1, 130), (3, 2, 7)]


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


def _elems(curve, count, arity, seed):
    """count x arity elements as integers, 0 and r - 1 in every position among the first rows"""
    xs = [pu.random_elems(curve, arity, seed + j) for j in range(count)]
    for pos in range(arity):
        if 2 * pos + 1 < count:
            xs[2 * pos][pos], xs[2 * pos + 1][pos] = 0, curve.fr.p - 1
    return xs, pu.limbs([e for x in xs for e in x]).reshape(count, arity, 4)


def _finish(backend, curve, full, Z, count, seed):
    keys = Groth16Keys(backend, full, seed=seed)
    r, s = _rs(curve, count, seed + 1)
    hr = backend.r1cs_upload(curve.cid, full.arrays())
    pk = keys.pk_dict()
    ref = [backend.groth16_prove_resident(curve.cid, pk, hr, Z[j], r[j], s[j]) for j in range(count)]
    return dict(full=full, keys=keys, Z=Z, r=r, s=s, hr=hr, pk=pk, ref=ref)


def _make_hash(backend, curve, arity, count, seed):
    xs, v = _elems(curve, count, arity, seed + 2)
    Z = poseidon_hash_assignments_host(curve.cid, v)  # (tests/test_poseidon_arity_assignments_cpu.py pins these rows to the compilers')
    m = _finish(backend, curve, Circuit.poseidon_hash(curve.cid, xs[0]), Z, count, seed)
    m.update(xs=xs, v=v, arity=arity)
    return m


def _make_leaf(backend, curve, arity, depth, count, seed):
    xs, v = _elems(curve, count, arity, seed + 2)
    paths = [pu.random_elems(curve, depth, seed + 500 + j) for j in range(count)]
    idx = [(5 * j + 1) % (1 << depth) for j in range(count)]
    idx[0] = 0
    if count > 2:
        idx[1] = (1 << depth) - 1
        paths[2][0] = 0
    ix = np.array(idx, dtype=np.uint64)
    pav = pu.limbs([e for row in paths for e in row]).reshape(count, depth, 4)
    Z = poseidon_merkle_leaf_assignments_host(curve.cid, v, ix, pav, depth)
    m = _finish(backend, curve, Circuit.merkle_leaf(curve.cid, depth, xs[0], idx[0], paths[0]), Z, count, seed)
    m.update(xs=xs, v=v, arity=arity, depth=depth, idx=idx, ix=ix, paths=paths, pav=pav)
    return m


@pytest.fixture(scope="module")
def made(backend):
    """per (curve, family, shape): keys, inputs, the host mirror's rows, blinding scalars and the resident prover's proof of each, made once and shared"""
    cache = {}

    def get(curve, family, *shape):
        key = (curve.cid, family) + shape
        if key not in cache:
            seed = 2100 + 97 * len(cache)
            count = dict(HASH_SHAPES)[shape[0]] if family == "hash" else {(a, d): n for a, d, n in LEAF_SHAPES}.get(shape, 7)
            cache[key] = _make_hash(backend, curve, shape[0], count, seed) if family == "hash" else _make_leaf(backend, curve, shape[0], shape[1], count, seed)
        return cache[key]

    yield get
    for m in cache.values():
        backend.r1cs_free(m["hr"])
        m["keys"].close()
        m["full"].close()


def _check(m, got, count):
    return len(got) == count and all(_same(got[j], m["ref"][j]) for j in range(count))


def _domain(m):
    return 1 << max(1, (m["full"].shape[0] + m["full"].shape[1] - 1).bit_length())


def _fallbacks(m):
    """the two settings that send a batch of 7 to the loop over the resident prover"""
    yield {"ZL_TUNE_G16_BATCH_LOG_N": str(_domain(m).bit_length() - 2), "ZL_TUNE_G16_BATCH_MIN": "1"}  # the domain bound below the circuit
    yield {"ZL_TUNE_G16_BATCH_LOG_N": "28", "ZL_TUNE_G16_BATCH_MIN": "8"}                              # the minimum count above the batch


def _run_everywhere(backend, m, device_path, prove, exp_pub, count):
    """the device path (in several chunks when the batch is large), then 7 proofs on both fallbacks with the rows from the device and from the host mirror"""
    got, pub = prove(count)
    assert _check(m, got, count) and np.array_equal(pub, exp_pub[:count])
    assert m["keys"].verify_batch(got, pub.reshape(count, 1, 4))
    with pytest.raises(BackendError) as e:
        backend.groth16_last_h(2)  # the device path ran: no single quotient
    assert e.value.code == EINVAL
    device_path.setenv("ZL_TUNE_G16_BATCH_CHUNK", "48" if count > 7 else "3")  # 48 + 48 + 34 proofs, or 3 + 3 + 1 ...
    device_path.setenv("ZL_TUNE_POSEIDON_CHUNK", "32" if count > 7 else "2")   # ... whose traces run as 32 + 16 (32 + 2), or 2 + 1
    got, pub = prove(count)
    assert _check(m, got, count) and np.array_equal(pub, exp_pub[:count])
    device_path.delenv("ZL_TUNE_G16_BATCH_CHUNK")
    device_path.delenv("ZL_TUNE_POSEIDON_CHUNK")
    n = _domain(m)
    for env in _fallbacks(m):
        for key, v in env.items():
            device_path.setenv(key, v)
        for dev_min in ("0", str(1 << 30)):
            device_path.setenv("ZL_TUNE_POSEIDON_DEV_MIN", dev_min)
            got, pub = prove(7)
            assert _check(m, got, 7) and np.array_equal(pub, exp_pub[:7])
            assert backend.groth16_last_h(n).shape == (n, 4)  # the resident prover ran and left its quotient


@CURVES
@pytest.mark.parametrize("arity,count", HASH_SHAPES)
def test_prove_hashes_equals_resident_on_every_path(backend, made, device_path, curve, arity, count):
    m = made(curve, "hash", arity)
    assert _domain(m) == 1 << 9 and m["keys"].hash_arity() == arity and m["keys"].merkle_leaf_shape() is None and m["keys"].chain_links() == 0
    assert pu.ints(m["Z"][:, 1]) == [pa.hash(curve, x) for x in m["xs"]]
    _run_everywhere(backend, m, device_path, lambda c: m["keys"].prove_hashes(m["v"][:c], m["r"][:c], m["s"][:c]), m["Z"][:, 1], count)


@CURVES
@pytest.mark.parametrize("arity,depth,count", LEAF_SHAPES)
def test_prove_leaf_paths_equals_resident_on_every_path(backend, made, device_path, curve, arity, depth, count):
    m = made(curve, "leaf", arity, depth)
    assert _domain(m) == 1 << 10 and m["keys"].merkle_leaf_shape() == (arity, depth) and m["keys"].hash_arity() == 0 and m["keys"].merkle_depth() == 0
    assert pu.ints(m["Z"][:, 1]) == [au.leaf_root(curve, m["xs"][j], m["idx"][j], m["paths"][j]) for j in range(count)]
    _run_everywhere(backend, m, device_path, lambda c: m["keys"].prove_merkle_leaf_paths(m["v"][:c], m["ix"][:c], m["pav"][:c], m["r"][:c], m["s"][:c]), m["Z"][:, 1],
                    count)


@CURVES
@pytest.mark.parametrize("family", ["hash", "leaf"])
def test_proof_equals_the_oracle_on_the_python_builders_matrices(backend, made, device_path, curve, family):
    """the wide gadget against the C oracle end to end: its matrices are the Python builder's, its key the queries the library's setup made"""
    j = 2
    if family == "hash":
        m = made(curve, "hash", 5)
        cs = au.poseidon_hash_circuit(curve.fr, m["xs"][j])
        prove = lambda sl: m["keys"].prove_hashes(m["v"][sl], m["r"][sl], m["s"][sl])
    else:
        m = made(curve, "leaf", 3, 2)  # the membership with a zero sibling
        cs = au.poseidon_merkle_leaf_circuit(curve.fr, 2, m["xs"][j], m["idx"][j], m["paths"][j])
        prove = lambda sl: m["keys"].prove_merkle_leaf_paths(m["v"][sl], m["ix"][sl], m["pav"][sl], m["r"][sl], m["s"][sl])
    assert cs.is_satisfied()
    z = ol.ints_to_limbs(cs.assignment(), 4)
    assert np.array_equal(z, m["Z"][j])
    pk = dict(m["pk"])
    for name in ("a_query", "b_g1_query", "h_query", "l_query", "b_g2_query"):
        pk[name] = backend.bases_download(m["pk"][name])
    exp, _ = gu.oracle_prove(curve, gu.r1cs_arrays(cs), z, pk, m["r"][j], m["s"][j], threads=8)
    got, pub = prove(slice(j, j + 1))  # the device path
    assert _same(got[0], exp) and np.array_equal(pub[0], z[1])


@CURVES
def test_errors(backend, made, device_path, curve):
    mh, ml = made(curve, "hash", 5), made(curve, "leaf", 3, 2)
    v, r, s = mh["v"][:4], mh["r"][:4], mh["s"][:4]
    lv, lix, lpa = ml["v"][:4], ml["ix"][:4], ml["pav"][:4]
    with pytest.raises(ValueError):  # keys of the other family are refused ...
        mh["keys"].prove_merkle_leaf_paths(lv, lix, lpa, r, s)
    with pytest.raises(ValueError):
        mh["keys"].prove_merkle_leaf_members(0, 0, 1, lix[:0], r[:0], s[:0])
    with pytest.raises(ValueError):
        ml["keys"].prove_hashes(v, r, s)
    chain, member = Circuit(curve.cid, 2), Circuit.merkle(curve.cid, 1, 1, 0, [2])
    others = [(c, Groth16Keys(backend, c, seed=9), backend.r1cs_upload(curve.cid, c.arrays())) for c in (chain, member)]
    try:
        for c, k, h in others:
            assert k.hash_arity() == 0 and k.merkle_leaf_shape() is None
            with pytest.raises(ValueError):
                k.prove_hashes(v, r, s)
            for arity in (2, 3, 4, 5):  # ... by the library too, at every arity it could be asked for
                w = np.ascontiguousarray(np.tile(v[:, :1], (1, arity, 1)))
                with pytest.raises(BackendError) as e:
                    backend.groth16_prove_poseidon_hashes(curve.cid, k.pk_dict(), h, arity, w, r, s)
                assert e.value.code == EINVAL
                with pytest.raises(BackendError) as e:
                    backend.groth16_prove_merkle_leaf_paths(curve.cid, k.pk_dict(), h, arity, 1, w, np.zeros(4, dtype=np.uint64), lpa[:, :1], r, s)
                assert e.value.code == EINVAL
    finally:
        for c, k, h in others:
            backend.r1cs_free(h)
            k.close()
            c.close()
    for log_n in ("28", "0"):  # on the device path and on the fallback
        device_path.setenv("ZL_TUNE_G16_BATCH_LOG_N", log_n)
        for arity in (0, 1, 3, 4, 6):  # an arity that is not the circuit's, arities outside 2..5
            w = np.ascontiguousarray(np.tile(v[:, :1], (1, max(1, arity), 1)))
            with pytest.raises(BackendError) as e:
                backend.groth16_prove_poseidon_hashes(curve.cid, mh["pk"], mh["hr"], arity, w, r, s)
            assert e.value.code == EINVAL
        with pytest.raises(BackendError) as e:  # hash keys at the leaf prover, leaf keys at the hash prover
            backend.groth16_prove_merkle_leaf_paths(curve.cid, mh["pk"], mh["hr"], 5, 1, v, lix, lpa[:, :1], r, s)
        assert e.value.code == EINVAL
        with pytest.raises(BackendError) as e:
            backend.groth16_prove_poseidon_hashes(curve.cid, ml["pk"], ml["hr"], 3, lv, r, s)
        assert e.value.code == EINVAL
        pa41 = np.ascontiguousarray(np.tile(lpa[:, :1], (1, 41, 1)))
        for arity, depth, paths in ((3, 1, lpa[:, :1]), (3, 3, pa41[:, :3]), (3, 0, lpa[:, :1]), (3, 41, pa41), (4, 2, lpa)):  # another depth, depths outside 1..40, another arity
            pre = lv if arity == 3 else np.ascontiguousarray(np.tile(lv[:, :1], (1, arity, 1)))
            with pytest.raises(BackendError) as e:
                backend.groth16_prove_merkle_leaf_paths(curve.cid, ml["pk"], ml["hr"], arity, depth, pre, lix, np.ascontiguousarray(paths), r, s)
            assert e.value.code == EINVAL
        with pytest.raises(BackendError) as e:
            backend.groth16_prove_poseidon_hashes(curve.cid, mh["pk"], 0x7FFF0001, 5, v, r, s)
        assert e.value.code == EHANDLE
        bad_ix = lix.copy()
        bad_ix[2] = 4  # == 2^depth
        with pytest.raises(BackendError) as e:
            ml["keys"].prove_merkle_leaf_paths(lv, bad_ix, lpa, r, s)
        assert e.value.code == EINVAL
        at_r = pu.limbs([curve.fr.p])[0]
        bad = v.copy()
        bad[2, 4] = at_r
        with pytest.raises(BackendError) as e:
            mh["keys"].prove_hashes(bad, r, s)
        assert e.value.code == EINVAL
        for which in ("preimage", "sibling"):
            bad_lv, bad_pa = lv.copy(), lpa.copy()
            if which == "preimage":
                bad_lv[2, 1] = at_r
            else:
                bad_pa[2, 1] = at_r
            with pytest.raises(BackendError) as e:
                ml["keys"].prove_merkle_leaf_paths(bad_lv, lix, bad_pa, r, s)
            assert e.value.code == EINVAL
        got, pub = mh["keys"].prove_hashes(v[:0], r[:0], s[:0])  # count == 0
        assert got == [] and pub.shape == (0, 4)
        got, roots = ml["keys"].prove_merkle_leaf_paths(lv[:0], lix[:0], lpa[:0], r[:0], s[:0])
        assert got == [] and roots.shape == (0, 4)
        got, pub = backend.groth16_prove_poseidon_hashes(curve.cid, mh["pk"], mh["hr"], 5, v, r, s)  # usable after the errors
        assert _check(mh, got, 4) and np.array_equal(pub, mh["Z"][:4, 1])
        got, roots = backend.groth16_prove_merkle_leaf_paths(curve.cid, ml["pk"], ml["hr"], 3, 2, lv, lix, lpa, ml["r"][:4], ml["s"][:4])
        assert _check(ml, got, 4) and np.array_equal(roots, ml["Z"][:4, 1])


@CURVES
def test_members_of_a_device_tree_prove_and_verify(backend, made, device_path, curve):
    """a 5-leaf tree of depth 3 (absent siblings at levels 0 and 1), its leaves hashed on the device from arity-3 preimages: the member form's proofs are the
    paths form's over the gathered paths on the device path and on the fallback, verify_batch accepts them with the returned root, and a preimage that does not
    hash to its leaf is refused"""
    arity, n, depth = 3, 5, 3
    m = made(curve, "leaf", arity, depth)
    assert m["keys"].merkle_leaf_shape() == (arity, depth) and _domain(m) == 1 << 10
    pre = m["v"][:n]
    d_pre = dev(pre)
    d_leaves = dev(np.zeros((n, 4), dtype=np.uint64))
    backend.poseidon_hash_dev(curve.cid, arity, d_pre.data_ptr(), n, d_leaves.data_ptr())
    d_nodes = dev(np.zeros((poseidon_merkle_nodes(n, depth), 4), dtype=np.uint64))
    root = backend.poseidon_merkle_build_dev(curve.cid, d_leaves.data_ptr(), n, depth, d_nodes.data_ptr())
    ix = np.array([4, 0, 3, 1, 2, 4, 4], dtype=np.uint64)
    r, s = _rs(curve, ix.size, 77)
    paths = backend.poseidon_merkle_paths(curve.cid, d_nodes.data_ptr(), n, depth, ix)
    exp, roots = m["keys"].prove_merkle_leaf_paths(pre[ix.astype(np.int64)], ix, paths, r, s)
    assert np.array_equal(roots, np.tile(root, (ix.size, 1)))
    Z = poseidon_merkle_leaf_assignments_host(curve.cid, pre[ix.astype(np.int64)], ix, paths, depth)
    assert all(_same(exp[j], backend.groth16_prove_resident(curve.cid, m["pk"], m["hr"], Z[j], r[j], s[j])) for j in range(ix.size))
    got, got_root = m["keys"].prove_merkle_leaf_members(d_nodes.data_ptr(), d_pre.data_ptr(), n, ix, r, s)
    assert len(got) == ix.size and all(_same(a, b) for a, b in zip(got, exp)) and np.array_equal(got_root, root)
    assert m["keys"].verify_batch(got, np.tile(got_root, (ix.size, 1)).reshape(ix.size, 1, 4))
    device_path.setenv("ZL_TUNE_G16_BATCH_CHUNK", "3")
    device_path.setenv("ZL_TUNE_POSEIDON_CHUNK", "2")
    got, got_root = m["keys"].prove_merkle_leaf_members(d_nodes.data_ptr(), d_pre.data_ptr(), n, ix, r, s)
    assert all(_same(a, b) for a, b in zip(got, exp)) and np.array_equal(got_root, root)
    device_path.setenv("ZL_TUNE_G16_BATCH_MIN", "8")  # the resident loop: the rows the device wrote come back through host staging
    got, got_root = m["keys"].prove_merkle_leaf_members(d_nodes.data_ptr(), d_pre.data_ptr(), n, ix, r, s)
    assert all(_same(a, b) for a, b in zip(got, exp)) and np.array_equal(got_root, root)
    assert backend.groth16_last_h(_domain(m)).shape == (_domain(m), 4)
    wrong = pre.copy()
    wrong[3, 2, 0] ^= np.uint64(1)
    assert pu.ints(wrong[3, 2])[0] < curve.fr.p
    d_wrong = dev(wrong)
    for batch_min in ("8", "1"):  # on the fallback and on the device path
        device_path.setenv("ZL_TUNE_G16_BATCH_MIN", batch_min)
        with pytest.raises(BackendError) as e:
            m["keys"].prove_merkle_leaf_members(d_nodes.data_ptr(), d_wrong.data_ptr(), n, ix, r, s)
        assert e.value.code == EINVAL
        for n_leaves, idx in ((5, [0, 5]), (9, [0, 1])):  # an index at n; more leaves than the depth holds
            with pytest.raises(BackendError) as e:
                m["keys"].prove_merkle_leaf_members(d_nodes.data_ptr(), d_pre.data_ptr(), n_leaves, idx, r[:2], s[:2])
            assert e.value.code == EINVAL
    got, got_root = m["keys"].prove_merkle_leaf_members(d_nodes.data_ptr(), d_pre.data_ptr(), n, ix[:2], r[:2], s[:2])  # usable after the errors
    assert all(_same(a, b) for a, b in zip(got, exp[:2])) and np.array_equal(got_root, root)
    got, got_root = m["keys"].prove_merkle_leaf_members(d_nodes.data_ptr(), d_pre.data_ptr(), n, [], r[:0], s[:0])
    assert got == []
