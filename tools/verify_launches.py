"""The verification calls whose kernel launches profiles/verify_refactor_ab.log compares between two builds (ZL_BACKEND_LIB selects the library):

  rocprofv3 --kernel-trace --stats -d OUT -- python tools/verify_launches.py

On both curves, over proofs of the 235-constraint Poseidon circuit and with a fixed seed for every combination: verify_batch accepted at 64 proofs; rejected
with each=True at 64 proofs (host final exponentiations) and at 256 (device: the default ZL_TUNE_FEXP_DEV_MIN is 128); pairing_products at 65 products of 2
pairs; verify_batch_bytes at 64 proofs.  Every result is asserted, so a run that launches the same kernels also computed the same verdicts."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openzl_amd import ZL_BLS12_381, ZL_BN254, ZL_G1, ZL_G2, Backend, Circuit, Groth16Keys  # noqa: E402
from openzl_amd.backend import proof_to_bytes  # noqa: E402


def main():
    be = Backend(0)
    for curve in (ZL_BLS12_381, ZL_BN254):
        circ = Circuit(curve, 1)
        keys = Groth16Keys(be, circ, seed=0xBE4C)
        pub = circ.arrays()["assignment"][1:2]
        proofs = keys.prove_many(list(range(256)))
        pubs = np.tile(pub[None], (256, 1, 1))
        assert keys.verify_batch(proofs[:64], pubs[:64], seed=7)
        for m in (64, 256):
            bad = pubs[:m].copy()
            bad[m // 2, 0, 0] ^= np.uint64(1)
            ok, each = keys.verify_batch(proofs[:m], bad, seed=7, each=True)
            assert not ok and [bool(e) for e in each] == [i != m // 2 for i in range(m)]
        rng = np.random.default_rng(3)
        k = rng.integers(0, 2 ** 63, size=(130, 4), dtype=np.uint64)
        k[:, 3] &= np.uint64((1 << 59) - 1)
        h1, h2 = be.bases_generate(curve, k, group=ZL_G1), be.bases_generate(curve, k[::-1].copy(), group=ZL_G2)
        P, Q = be.bases_download(h1), be.bases_download(h2)
        be.bases_free(h1)
        be.bases_free(h2)
        got, st = be.pairing_products(curve, P, Q, 2)
        assert not st.any() and (got[64] == be.pairing_product(curve, P[128:130], Q[128:130])).all()
        data = b"".join(proof_to_bytes(curve, p) for p in proofs[:64])
        ok, each, st = keys.verify_batch_bytes(data, 64, pubs[:64], seed=7, each=True)
        assert ok and each.all() and not st.any()
        keys.close()
    be.close()
    print("verify_launches ok")


if __name__ == "__main__":
    main()
