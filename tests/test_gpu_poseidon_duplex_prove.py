"""The duplex-encryption circuit through the EXISTING Groth16 provers, and the tie between the cipher kernel and the circuit: keys compiled from the full
circuit of one message (width 3, key of 2, no header, one block), five other messages proven from witness-only circuits through prove_batch, every proof equal to
the resident prover's for the same assignment, and verify_batch accepting them with the public inputs [tag, c0, c1] that poseidon_duplex_encrypt computed ON THE
DEVICE -- and refusing them once one ciphertext element is changed."""
import numpy as np
import pytest

import oracle_lib as ol
import poseidon_duplex_util as du
import poseidon_util as pu
from openzl_amd import Circuit, Groth16Keys

pytestmark = pytest.mark.gpu

WIDTH, SHAPE, COUNT = 3, (2, 0, 1), 5


def _same(p, q):
    return all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(p, q))


@pytest.mark.parametrize("curve", pu.CURVES, ids=lambda c: c.name)
def test_encryptions_prove_and_verify_against_the_device_cipher(backend, curve, monkeypatch):
    monkeypatch.setenv("ZL_TUNE_POSEIDON_DEV_MIN", "0")
    monkeypatch.setenv("ZL_TUNE_G16_BATCH_MIN", "1")
    p = curve.fr.p
    st = pu.random_elems(curve, WIDTH, 21)
    items = du.random_items(curve, WIDTH, SHAPE, COUNT + 1, 22)
    items[1] = ([p - 1, 0], [], [[p - 1, 0]])
    full = Circuit.poseidon_encrypt(curve.cid, st, *items[0])
    assert full.shape == du.circuit_shape(WIDTH, *SHAPE) == (948, 4, 949)
    keys = Groth16Keys(backend, full, seed=31)
    hr = backend.r1cs_upload(curve.cid, full.arrays())
    try:
        Z = []
        for it in items[1:]:
            w = Circuit.poseidon_encrypt(curve.cid, st, *it, witness_only=True)
            try:
                Z.append(w.arrays()["assignment"])
            finally:
                w.close()
        Z = np.ascontiguousarray(np.stack(Z))
        rs = ol.random_scalars(curve, 2 * COUNT, 32)
        r, s = np.ascontiguousarray(rs[:COUNT]), np.ascontiguousarray(rs[COUNT:])
        proofs = keys.prove_batch(Z, r, s)
        pk = keys.pk_dict()
        assert all(_same(proofs[j], backend.groth16_prove_resident(curve.cid, pk, hr, Z[j], r[j], s[j])) for j in range(COUNT))
        k, h, t = du.pack(items[1:], WIDTH, SHAPE)
        ct, tags = backend.poseidon_duplex_encrypt(curve.cid, pu.limbs(st), k, h, t)
        pub = np.ascontiguousarray(np.concatenate([tags.reshape(COUNT, 1, 4), ct.reshape(COUNT, 2, 4)], axis=1))
        assert pub.tobytes() == Z[:, 1:4].tobytes()
        assert keys.verify_batch(proofs, pub, seed=33)
        bad = pub.copy()
        bad[2, 1] = pu.limbs([(pu.ints(bad[2, 1])[0] + 1) % p])[0]
        ok, each = keys.verify_batch(proofs, bad, seed=33, each=True)
        assert not ok and list(each) == [j != 2 for j in range(COUNT)]
    finally:
        backend.r1cs_free(hr)
        keys.close()
        full.close()
