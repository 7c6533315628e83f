"""zl_groth16_prove_hybrid_encryptions: generator, ephemeral keys, public keys, headers and plaintexts in, proofs out -- k_ed_hybrid_ladders and
k_pos_duplex_trace_in write the assignments of the hybrid-encryption circuit straight into the batch's block and hand out epk, tag and ciphertext beside them.
bits = 8 at (W; H, N) = (3; 0, 1) has a domain of 2^11: 70 proofs take the device batch path under the library's own dispatch bounds, in several chunks; full
width loops the resident prover.  In both every proof equals zl_groth16_prove_resident on the host mirror's row with the same (r, s) byte for byte, the outputs
equal Backend.hybrid_encrypt's (another kernel path), and the batch verifies against publics assembled from those -- and not with one ciphertext element
changed; both fallbacks; keys of another width, of a scalar multiplication and of an encryption are refused."""
import numpy as np
import pytest

import edwards_util as eu
import hybrid_circuit_util as hu
import oracle_lib as ol
import poseidon_util as pu
from openzl_amd import BackendError, Circuit, Groth16Keys, ed_order_bits, hybrid_encrypt_assignments_host

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
EINVAL = -1
SHAPE = (3, 0, 1)


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
    w, h, n = SHAPE
    l = eu.params(curve)[3]
    top = min(l, 1 << bits)
    first = hu.item(curve, SHAPE, bits, seed)
    st, g = first[0], first[1]
    pool = [eu.ID, eu.small_order_points(curve)[2]] + eu.subgroup_points(curve, 2, seed + 5) + eu.random_points(curve, 2, seed + 6)
    esks = ([top - 1, 0, 1] + [k % top for k in eu.random_scalars(curve, count, seed + 7)])[:count]
    items = [(st, g) + hu.item(curve, SHAPE, bits, seed + 10 + i, esk=esks[i], pk=pool[(i + 2) % len(pool)])[2:] for i in range(count)]
    o = hu.words(items, w)
    rows = hybrid_encrypt_assignments_host(curve.cid, o["st"], o["g"], o["esk"], o["pk"], o["h"], o["t"], bits)
    full = Circuit.hybrid_encrypt(curve.cid, *items[0][:3], *items[0][4:], bits)
    assert np.array_equal(full.arrays()["assignment"], rows[0])
    keys = Groth16Keys(backend, full, seed=seed)
    r, s = _rs(curve, count, seed + 3)
    hr = backend.r1cs_upload(curve.cid, full.arrays())
    ref = [backend.groth16_prove_resident(curve.cid, keys.pk_dict(), hr, rows[j], r[j], s[j]) for j in range(count)]
    epk, ct, tag, status = backend.hybrid_encrypt(curve.cid, o["st"], o["g"], o["esk"], o["pk"], o["h"], o["t"])
    assert not status.any()
    t = n * (w - 1)
    pub = np.concatenate([np.tile(o["g"], (count, 1, 1)), o["pk"], epk, tag.reshape(count, 1, 4), ct.reshape(count, t, 4), o["h"]], axis=1)
    assert np.array_equal(pub, rows[:, 1:8 + t + h])
    return dict(full=full, keys=keys, r=r, s=s, hr=hr, ref=ref, o=o, epk=epk, ct=ct, tag=tag, pub=pub, bits=bits, count=count)


@pytest.fixture(scope="module")
def made(backend):
    """per (curve, bits): keys, inputs, the host mirror's rows, blinding scalars and the resident prover's proof of each, made once"""
    cache = {}

    def get(curve, bits, count):
        key = (curve.cid, bits)
        if key not in cache:
            cache[key] = _make(backend, curve, bits, count, 6100 + 37 * len(cache))
        return cache[key]

    yield get
    for m in cache.values():
        backend.r1cs_free(m["hr"])
        m["keys"].close()
        m["full"].close()


def _domain(m):
    return 1 << max(1, (m["full"].shape[0] + m["full"].shape[1] - 1).bit_length())


def _prove(m, c, keys=None, bits=None, pk=None):
    o = m["o"]
    return (keys or m["keys"]).prove_hybrid_encryptions(o["st"], o["g"], o["esk"][:c], o["pk"][:c] if pk is None else pk, o["h"][:c], o["t"][:c], m["r"][:c], m["s"][:c],
                                                        bits=m["bits"] if bits is None else bits)


def _ok(m, out, count):
    got, epk, tag, ct = out
    return (len(got) == count and all(_same(got[j], m["ref"][j]) for j in range(count)) and np.array_equal(epk, m["epk"][:count]) and np.array_equal(tag, m["tag"][:count])
            and np.array_equal(ct, m["ct"][:count]))


def _verifies(m, proofs, count):
    pub = m["pub"][:count]
    bad = pub[:1].copy()
    bad[0, 7, 1] ^= np.uint64(1)  # one flipped bit in the second word of the first ciphertext element (pub[0] is G.x: element 8 of the row); it stays below r
    return m["keys"].verify_batch(proofs, pub) and not m["keys"].verify_batch(proofs[:1], bad)


@CURVES
def test_eight_bits_take_the_device_batch_path_in_chunks(backend, made, monkeypatch, curve):
    m = made(curve, 8, 70)
    assert m["full"].shape == hu.shape(3, 8, 0, 1) and _domain(m) <= 1 << 11  # 64 proofs or more of this key take the device batch path
    out = _prove(m, 70)  # the library's own dispatch
    assert _ok(m, out, 70)
    with pytest.raises(BackendError) as e:
        backend.groth16_last_h(2)  # the device path ran: no single quotient
    assert e.value.code == EINVAL
    assert _verifies(m, out[0], 70)
    monkeypatch.setenv("ZL_TUNE_G16_BATCH_CHUNK", "30")  # 30 + 30 + 10 proofs ...
    monkeypatch.setenv("ZL_TUNE_ED_CHUNK", "64")         # ... (the traces of a chunk in one launch pair)
    assert _ok(m, _prove(m, 70), 70)
    monkeypatch.delenv("ZL_TUNE_G16_BATCH_CHUNK")
    monkeypatch.delenv("ZL_TUNE_ED_CHUNK")
    # one public key for all items
    o = m["o"]
    got, epk, tag, ct = _prove(m, 70, pk=o["pk"][5])
    e_epk, e_ct, e_tag, _ = backend.hybrid_encrypt(curve.cid, o["st"], o["g"], o["esk"][:70], o["pk"][5], o["h"][:70], o["t"][:70])
    assert np.array_equal(epk, e_epk) and np.array_equal(tag, e_tag) and np.array_equal(ct, e_ct)
    pub = np.concatenate([np.tile(o["g"], (70, 1, 1)), np.tile(o["pk"][5], (70, 1, 1)), epk, tag.reshape(70, 1, 4), ct.reshape(70, 2, 4)], axis=1)
    assert m["keys"].verify_batch(got, pub)
    assert _same(got[5], m["ref"][5])  # (item 5 has that key)
    got, epk, tag, ct = _prove(m, 0)
    assert got == [] and epk.shape == (0, 2, 4) and tag.shape == (0, 4) and ct.shape == (0, 1, 2, 4)


@CURVES
def test_both_fallbacks_loop_the_resident_prover(backend, made, monkeypatch, curve):
    m = made(curve, 8, 70)
    n = _domain(m)
    assert _ok(m, _prove(m, 7), 7)  # a count below ZL_TUNE_G16_BATCH_MIN
    assert backend.groth16_last_h(n).shape == (n, 4)  # the resident prover ran and left its quotient
    monkeypatch.setenv("ZL_TUNE_G16_BATCH_LOG_N", str(n.bit_length() - 2))  # the domain bound below the circuit
    monkeypatch.setenv("ZL_TUNE_G16_BATCH_MIN", "1")
    for dev_min in ("0", str(1 << 30)):  # the rows from the two launches through host staging, and from the host mirror
        monkeypatch.setenv("ZL_TUNE_ED_DEV_MIN", dev_min)
        out = _prove(m, 66)
        assert _ok(m, out, 66)
        assert backend.groth16_last_h(n).shape == (n, 4)
    assert _verifies(m, out[0], 66)


@CURVES
def test_full_width_loops_the_resident_prover(backend, made, monkeypatch, curve):
    bits = ed_order_bits(curve.cid)
    m = made(curve, bits, 3)
    n = _domain(m)
    assert m["full"].shape == hu.shape(3, bits, 0, 1) and n == 8192
    for dev_min in ("0", str(1 << 30)):
        monkeypatch.setenv("ZL_TUNE_ED_DEV_MIN", dev_min)
        out = _prove(m, 3)
        assert _ok(m, out, 3)
        assert backend.groth16_last_h(n).shape == (n, 4)
    assert _verifies(m, out[0], 3)
    # bits defaults to the full width
    o = m["o"]
    assert _ok(m, m["keys"].prove_hybrid_encryptions(o["st"], o["g"], o["esk"], o["pk"], o["h"], o["t"], m["r"], m["s"]), 3)


@CURVES
def test_wrong_keys_are_refused(backend, made, curve):
    m = made(curve, 8, 70)
    o = m["o"]
    it9 = hu.item(curve, SHAPE, 9, 77)
    others = [Circuit.hybrid_encrypt(curve.cid, *it9[:3], *it9[4:], 9),                                 # keys of bits 9 used for bits 8
              Circuit.ed_scalar_mul(curve.cid, eu.subgroup_points(curve, 1, 78)[0], 5, 8),               # keys of a scalar multiplication
              Circuit.poseidon_encrypt(curve.cid, None, [1, 2], [], [[3, 4]])]                           # keys of an encryption
    for c in others:
        k = Groth16Keys(backend, c, seed=9)
        try:
            with pytest.raises(BackendError) as e:
                _prove(m, 4, keys=k)
            assert e.value.code == EINVAL
        finally:
            k.close()
            c.close()
    for bits in (7, 9, ed_order_bits(curve.cid), 0, 253):
        with pytest.raises(BackendError) as e:
            _prove(m, 4, bits=bits)
        assert e.value.code == EINVAL, bits
    bad = o["esk"][:4].copy()
    bad[2] = pu.limbs([1 << 8])[0]
    with pytest.raises(BackendError) as e:  # an ephemeral key of 9 bits
        m["keys"].prove_hybrid_encryptions(o["st"], o["g"], bad, o["pk"][:4], o["h"][:4], o["t"][:4], m["r"][:4], m["s"][:4], bits=8)
    assert e.value.code == EINVAL
    assert _ok(m, _prove(m, 4), 4)  # usable after the errors
