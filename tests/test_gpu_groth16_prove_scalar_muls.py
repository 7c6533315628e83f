"""zl_groth16_prove_ed_scalar_muls: points and scalars in, proofs out -- k_ed_mul_trace writes the assignments of the scalar-multiplication circuit straight into
the batch's block and hands out Q beside them.  bits = 16 with 66 proofs takes the device batch path under the library's own dispatch bounds, in two chunks;
full width (a domain of 2^12) loops the resident prover.  In both every proof equals zl_groth16_prove_resident on the COMPILER's assignment with the same (r,
s) byte for byte, Q equals the batched multiplication's, and the batch verifies against (P, Q); keys of another `bits` are refused."""
import numpy as np
import pytest

import edwards_util as eu
import oracle_lib as ol
import poseidon_util as pu
from openzl_amd import BackendError, Circuit, Groth16Keys, ed_order_bits, ed_scalar_mul_host

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
EINVAL = -1


def _same(p, q):
    return all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(p, q))


def _rs(curve, count, seed):
    """distinct blinding scalars with one r and one s zero"""
    rs = ol.random_scalars(curve, 2 * count, seed)
    r, s = np.ascontiguousarray(rs[:count]), np.ascontiguousarray(rs[count:])
    r[min(3, count - 1)] = 0
    s[min(4, count - 1)] = 0
    return r, s


def _make(backend, curve, bits, count, seed):
    l = eu.params(curve)[3]
    top = min(l, 1 << bits)
    pool = [eu.ID, eu.small_order_points(curve)[2]] + eu.subgroup_points(curve, 2, seed) + eu.random_points(curve, 2, seed + 1)
    pts = [pool[(i + 2) % len(pool)] for i in range(count)]
    ks = ([top - 1, 0, 1] + [k % top for k in eu.random_scalars(curve, count, seed + 2)])[:count]
    Z = []
    for pt, k in zip(pts, ks):  # the compiler's assignment of every item
        c = Circuit.ed_scalar_mul(curve.cid, pt, k, bits, witness_only=True)
        Z.append(c.arrays()["assignment"])
        c.close()
    full = Circuit.ed_scalar_mul(curve.cid, pts[0], ks[0], bits)
    keys = Groth16Keys(backend, full, seed=seed)
    r, s = _rs(curve, count, seed + 3)
    hr = backend.r1cs_upload(curve.cid, full.arrays())
    ref = [backend.groth16_prove_resident(curve.cid, keys.pk_dict(), hr, Z[j], r[j], s[j]) for j in range(count)]
    p, k = eu.point_words(pts), pu.limbs(ks)
    q, status = ed_scalar_mul_host(curve.cid, p, k)
    assert not status.any()
    return dict(full=full, keys=keys, r=r, s=s, hr=hr, ref=ref, p=p, k=k, q=q, bits=bits, count=count)


@pytest.fixture(scope="module")
def made(backend):
    """per (curve, bits): keys, inputs, the compilers' rows, blinding scalars and the resident prover's proof of each, made once"""
    cache = {}

    def get(curve, bits, count):
        key = (curve.cid, bits)
        if key not in cache:
            cache[key] = _make(backend, curve, bits, count, 5200 + 31 * len(cache))
        return cache[key]

    yield get
    for m in cache.values():
        backend.r1cs_free(m["hr"])
        m["keys"].close()
        m["full"].close()


def _domain(m):
    return 1 << max(1, (m["full"].shape[0] + m["full"].shape[1] - 1).bit_length())


def _ok(m, out, count):
    got, q = out
    return len(got) == count and all(_same(got[j], m["ref"][j]) for j in range(count)) and np.array_equal(q, m["q"][:count])


def _prove(m, c):
    return m["keys"].prove_scalar_muls(m["p"][:c], m["k"][:c], m["r"][:c], m["s"][:c], bits=m["bits"])


def _verifies(m, proofs, count):
    pub = np.concatenate([m["p"][:count], m["q"][:count]], axis=1)
    bad = pub[:1].copy()
    bad[0, 3, 0] ^= np.uint64(1)  # one flipped word of Q.y (the identity's Q.y = 1 becomes 0; every other value stays below q: q is odd and Q.y is not q - 1 + 1)
    return m["keys"].verify_batch(proofs, pub) and not m["keys"].verify_batch(proofs[:1], bad)


@CURVES
def test_sixteen_bits_take_the_device_batch_path_in_two_chunks(backend, made, monkeypatch, curve):
    m = made(curve, 16, 66)
    assert m["full"].shape == (14 * 16 - 8, 5, 14 * 16 - 10) and _domain(m) == 256
    out = _prove(m, 66)  # the library's own dispatch: a domain below 2^11 and 64 proofs or more
    assert _ok(m, out, 66)
    with pytest.raises(BackendError) as e:
        backend.groth16_last_h(2)  # the device path ran: no single quotient
    assert e.value.code == EINVAL
    assert _verifies(m, out[0], 66)
    monkeypatch.setenv("ZL_TUNE_G16_BATCH_CHUNK", "40")  # 40 + 26 proofs ...
    monkeypatch.setenv("ZL_TUNE_ED_CHUNK", "64")         # ... (the traces of a chunk in one launch)
    assert _ok(m, _prove(m, 66), 66)
    monkeypatch.delenv("ZL_TUNE_G16_BATCH_CHUNK")
    monkeypatch.delenv("ZL_TUNE_ED_CHUNK")
    # one point for all items
    got, q = m["keys"].prove_scalar_muls(m["p"][5], m["k"][:66], m["r"][:66], m["s"][:66], bits=16)
    exp_q, _ = ed_scalar_mul_host(curve.cid, m["p"][5], m["k"][:66])
    assert np.array_equal(q, exp_q)
    assert m["keys"].verify_batch(got, np.concatenate([np.tile(m["p"][5], (66, 1, 1)), q], axis=1))
    assert _same(got[5], m["ref"][5])  # (item 5 has that point)
    # below 64 proofs: the loop over the resident prover
    assert _ok(m, _prove(m, 7), 7)
    assert backend.groth16_last_h(256).shape == (256, 4)
    got, q = _prove(m, 0)
    assert got == [] and q.shape == (0, 2, 4)


@CURVES
def test_full_width_loops_the_resident_prover(backend, made, monkeypatch, curve):
    bits = ed_order_bits(curve.cid)
    m = made(curve, bits, 3)
    assert m["full"].shape == (14 * bits - 8, 5, 14 * bits - 10) and _domain(m) == 4096
    for dev_min in ("0", str(1 << 30)):  # the rows from the trace kernel through host staging, and from the host mirror
        monkeypatch.setenv("ZL_TUNE_ED_DEV_MIN", dev_min)
        out = _prove(m, 3)
        assert _ok(m, out, 3)
        assert backend.groth16_last_h(4096).shape == (4096, 4)  # the resident prover ran and left its quotient
    assert _verifies(m, out[0], 3)
    # bits defaults to the full width
    assert _ok(m, m["keys"].prove_scalar_muls(m["p"], m["k"], m["r"], m["s"]), 3)


@CURVES
def test_keys_of_another_width_are_refused(backend, made, curve):
    m = made(curve, 16, 66)
    p, k, r, s = m["p"][:4], m["k"][:4], m["r"][:4], m["s"][:4]
    for bits in (15, 17, ed_order_bits(curve.cid), 0, 253):
        with pytest.raises(BackendError) as e:
            m["keys"].prove_scalar_muls(p, k, r, s, bits=bits)
        assert e.value.code == EINVAL, bits
    hash_c = Circuit.poseidon_hash(curve.cid, [1, 2])
    hash_k = Groth16Keys(backend, hash_c, seed=9)
    try:
        with pytest.raises(BackendError) as e:  # keys of a hash circuit
            hash_k.prove_scalar_muls(p, k, r, s, bits=16)
        assert e.value.code == EINVAL
    finally:
        hash_k.close()
        hash_c.close()
    bad_k = k.copy()
    bad_k[2] = pu.limbs([1 << 16])[0]
    with pytest.raises(BackendError) as e:  # a scalar of 17 bits
        m["keys"].prove_scalar_muls(p, bad_k, r, s, bits=16)
    assert e.value.code == EINVAL
    assert _ok(m, _prove(m, 4), 4)  # usable after the errors
