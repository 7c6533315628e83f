"""zl_groth16_prove_poseidon_encryptions: keys, headers and plaintexts in, proofs out -- k_pos_duplex_trace writes the assignments of the encryption circuit
straight into the batch's block and hands out tag and ciphertext beside them.  Every proof must equal zl_groth16_prove_resident for the same (host-mirror row,
r, s) byte for byte, on the device path (forced with ZL_TUNE_G16_BATCH_LOG_N / _MIN), in several chunks, and on both fallbacks to the loop over the resident
prover; tags and ciphertexts equal the cipher's; the batch verifies against publics taken from the cipher call; keys of another shape are refused; and rows made
by zl_poseidon_encrypt_assignments_dev, fed to zl_groth16_prove_batch_dev, give the same proofs."""
import numpy as np
import pytest

import oracle_lib as ol
import poseidon_duplex_util as du
import poseidon_util as pu
from openzl_amd import BackendError, Circuit, Groth16Keys, poseidon_encrypt_assignment_elems, poseidon_encrypt_assignments_host

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
EINVAL, EHANDLE = -1, -5
# (width, (K, H, N), proofs, log2 of the domain): the reference test's shape E over several chunks; shape A at width 3; a full header block at width 6
SHAPES = [(4, (2, 0, 1), 130, 10), (3, (1, 0, 1), 7, 10), (6, (1, 5, 1), 7, 11)]


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


def _make(backend, curve, width, shape, count, seed):
    st = pu.random_elems(curve, width, seed + 3)
    stw = pu.limbs(st)
    items = (du.bound_items(curve, width, shape) + du.random_items(curve, width, shape, count, seed + 2))[:count]
    k, h, t = du.pack(items, width, shape)
    Z = poseidon_encrypt_assignments_host(curve.cid, stw, k, h, t)  # (tests/test_poseidon_encrypt_assignments_cpu.py pins these rows to the compilers')
    full = Circuit.poseidon_encrypt(curve.cid, st, *items[0])
    keys = Groth16Keys(backend, full, seed=seed)
    r, s = _rs(curve, count, seed + 1)
    hr = backend.r1cs_upload(curve.cid, full.arrays())
    pk = keys.pk_dict()
    ref = [backend.groth16_prove_resident(curve.cid, pk, hr, Z[j], r[j], s[j]) for j in range(count)]
    cts, tags = backend.poseidon_duplex_encrypt(curve.cid, stw, k, h, t)
    return dict(full=full, keys=keys, Z=Z, r=r, s=s, hr=hr, pk=pk, ref=ref, st=st, stw=stw, items=items, k=k, h=h, t=t, cts=cts, tags=tags, width=width, shape=shape)


@pytest.fixture(scope="module")
def made(backend):
    """per (curve, width, shape): keys, inputs, the host mirror's rows, blinding scalars, the resident prover's proof of each and the cipher's outputs, made once"""
    cache = {}

    def get(curve, width, shape):
        key = (curve.cid, width, shape)
        if key not in cache:
            count = {(w, sh): n for w, sh, n, _ in SHAPES}[(width, shape)]
            cache[key] = _make(backend, curve, width, shape, count, 3100 + 97 * len(cache))
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


def _publics(m, count):
    """(tag, ciphertext, header) per proof, from the CIPHER call"""
    return np.concatenate([m["tags"][:count, None], m["cts"][:count].reshape(count, -1, 4), m["h"][:count]], axis=1)


def _prove(m, c):
    return m["keys"].prove_encryptions(m["stw"], m["k"][:c], m["h"][:c], m["t"][:c], m["r"][:c], m["s"][:c])


def _ok(m, out, count):
    got, tags, cts = out
    return _check(m, got, count) and np.array_equal(tags, m["tags"][:count]) and np.array_equal(cts, m["cts"][:count])


@CURVES
@pytest.mark.parametrize("width,shape,count,log_n", SHAPES)
def test_prove_encryptions_equals_resident_on_every_path(backend, made, device_path, curve, width, shape, count, log_n):
    m = made(curve, width, shape)
    k, h, n = shape
    assert _domain(m) == 1 << log_n and m["full"].shape == du.circuit_shape(width, k, h, n) and m["Z"].shape[1] == poseidon_encrypt_assignment_elems(width, k, h, n)
    assert np.array_equal(m["Z"][:, 1], m["tags"]) and np.array_equal(m["Z"][:, 2:2 + n * (width - 1)], m["cts"].reshape(count, -1, 4))
    out = _prove(m, count)  # the device path
    assert _ok(m, out, count)
    pub = _publics(m, count)
    assert m["keys"].verify_batch(out[0], pub)
    bad = pub[:1].copy()
    bad[0, 2, 0] ^= np.uint64(1)  # one flipped word of a ciphertext element -- the second public input after the tag (r is odd: r - 1 is the one value this could push to r)
    if pu.ints(bad[0, 2:3])[0] >= curve.fr.p:
        bad[0, 2, 0] ^= np.uint64(3)
    assert not m["keys"].verify_batch(out[0][:1], bad)
    with pytest.raises(BackendError) as e:
        backend.groth16_last_h(2)  # the device path ran: no single quotient
    assert e.value.code == EINVAL
    device_path.setenv("ZL_TUNE_G16_BATCH_CHUNK", "48" if count > 7 else "3")  # 48 + 48 + 34 proofs, or 3 + 3 + 1 ...
    device_path.setenv("ZL_TUNE_POSEIDON_CHUNK", "32" if count > 7 else "2")   # ... whose traces run as 32 + 16 (32 + 2), or 2 + 1
    assert _ok(m, _prove(m, count), count)
    device_path.delenv("ZL_TUNE_G16_BATCH_CHUNK")
    device_path.delenv("ZL_TUNE_POSEIDON_CHUNK")
    dom = _domain(m)
    for env in ({"ZL_TUNE_G16_BATCH_LOG_N": str(log_n - 1), "ZL_TUNE_G16_BATCH_MIN": "1"},   # the domain bound below the circuit
                {"ZL_TUNE_G16_BATCH_LOG_N": "28", "ZL_TUNE_G16_BATCH_MIN": "8"}):            # the minimum count above the batch
        for key, v in env.items():
            device_path.setenv(key, v)
        for dev_min in ("0", str(1 << 30)):  # the rows from the device through host staging, and from the host mirror
            device_path.setenv("ZL_TUNE_POSEIDON_DEV_MIN", dev_min)
            assert _ok(m, _prove(m, 7), 7)
            assert backend.groth16_last_h(dom).shape == (dom, 4)  # the resident prover ran and left its quotient


@CURVES
def test_assignments_dev_rows_feed_prove_batch_dev(backend, made, device_path, curve):
    width, shape, count, _ = SHAPES[0]
    m = made(curve, width, shape)
    k, h, n = shape
    nv = m["Z"].shape[1]
    d_k, d_h, d_t = dev(m["k"]), dev(m["h"].reshape(-1, 4) if h else np.zeros((1, 4), dtype=np.uint64)), dev(m["t"])
    d_rows = dev(np.zeros((count, nv, 4), dtype=np.uint64))
    backend.poseidon_encrypt_assignments_dev(curve.cid, width, m["stw"], d_k.data_ptr(), k, d_h.data_ptr(), h, d_t.data_ptr(), n, count, d_rows.data_ptr())
    assert np.array_equal(d_rows.cpu().numpy().view(np.uint64).reshape(count, nv, 4), m["Z"])
    got = m["keys"].prove_batch_dev(d_rows.data_ptr(), count, m["r"], m["s"])
    assert _check(m, got, count)


@CURVES
def test_errors(backend, made, device_path, curve):
    width, shape, _, _ = SHAPES[1]
    m = made(curve, width, shape)
    other = made(curve, *SHAPES[0][:2])
    k, h, t, r, s = m["k"][:4], m["h"][:4], m["t"][:4], m["r"][:4], m["s"][:4]
    hash_c = Circuit.poseidon_hash(curve.cid, [1, 2])
    hash_k = Groth16Keys(backend, hash_c, seed=9)
    hash_h = backend.r1cs_upload(curve.cid, hash_c.arrays())
    try:
        for log_n in ("28", "0"):  # on the device path and on the fallback
            device_path.setenv("ZL_TUNE_G16_BATCH_LOG_N", log_n)
            with pytest.raises(BackendError) as e:  # keys of a hash circuit
                backend.groth16_prove_poseidon_encryptions(curve.cid, hash_k.pk_dict(), hash_h, m["stw"], k, h, t, r, s)
            assert e.value.code == EINVAL
            with pytest.raises(BackendError) as e:  # keys of an encryption circuit of another (W, K, H, N)
                other["keys"].prove_encryptions(m["stw"], k, h, t, r, s)
            assert e.value.code == EINVAL
            with pytest.raises(BackendError) as e:  # the same width, another key length
                m["keys"].prove_encryptions(m["stw"], np.ascontiguousarray(np.tile(k, (1, 2, 1))), h, t, r, s)
            assert e.value.code == EINVAL
            with pytest.raises(BackendError) as e:  # no key
                m["keys"].prove_encryptions(m["stw"], k[:, :0], h, t, r, s)
            assert e.value.code == EINVAL
            with pytest.raises(BackendError) as e:
                backend.groth16_prove_poseidon_encryptions(curve.cid, m["pk"], 0x7FFF0001, m["stw"], k, h, t, r, s)
            assert e.value.code == EHANDLE
            at_r = pu.limbs([curve.fr.p])[0]
            for which in ("key", "text", "state"):
                bk, bt, bst = k.copy(), t.copy(), m["stw"].copy()
                if which == "key":
                    bk[2, 0] = at_r
                elif which == "text":
                    bt[2, 0, 1] = at_r
                else:
                    bst[1] = at_r
                with pytest.raises(BackendError) as e:
                    m["keys"].prove_encryptions(bst, bk, h, bt, r, s)
                assert e.value.code == EINVAL, which
            got, tags, cts = m["keys"].prove_encryptions(m["stw"], k[:0], h[:0], t[:0], r[:0], s[:0])  # count == 0
            assert got == [] and tags.shape == (0, 4) and cts.shape == (0,) + t.shape[1:]
            assert _ok(m, m["keys"].prove_encryptions(m["stw"], k, h, t, r, s), 4)  # usable after the errors
    finally:
        backend.r1cs_free(hash_h)
        hash_k.close()
        hash_c.close()
