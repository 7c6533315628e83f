"""Throughput of the device product of pairings and of batched Groth16 verification.

  python tools/pairing_bench.py [--quick]

Times zl_pairing_product at 2^10 / 2^14 / 2^16 pairs (pairs/s), Groth16Keys.verify_batch over 64 / 1 024 / 16 384 proofs of the 235-constraint Poseidon
circuit (proofs/s, OS-drawn combination as in production), and the host Groth16::verify loop over the first 64 of those proofs, on both curves.  Each
figure is the median of three timed calls after one warm-up call.  Prints one line per measurement and a JSON summary line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openzl_amd import ZL_BLS12_381, ZL_BN254, ZL_G1, ZL_G2, Backend, Circuit, Groth16Keys  # noqa: E402

NAMES = {ZL_BLS12_381: "bls12_381", ZL_BN254: "bn254"}
R = {ZL_BLS12_381: 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001,
     ZL_BN254: 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001}


def scalars(curve, n, seed):
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 2 ** 63, size=(n, 4), dtype=np.uint64)
    out[:, 3] &= np.uint64((1 << 59) - 1)  # < 2^251 < r
    return out


def timed(fn, reps=3):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="smallest sizes only (a smoke run of the tool)")
    args = ap.parse_args()
    be = Backend(0)
    print(be.describe(), flush=True)
    res = {}
    pair_sizes = [1 << 10] if args.quick else [1 << 10, 1 << 14, 1 << 16]
    batch_sizes = [64] if args.quick else [64, 1024, 16384]
    for curve in (ZL_BLS12_381, ZL_BN254):
        name = NAMES[curve]
        nmax = max(pair_sizes)
        h1 = be.bases_generate(curve, scalars(curve, nmax, 1), group=ZL_G1)
        h2 = be.bases_generate(curve, scalars(curve, nmax, 2), group=ZL_G2)
        P, Q = be.bases_download(h1), be.bases_download(h2)
        be.bases_free(h1)
        be.bases_free(h2)
        for n in pair_sizes:
            t = timed(lambda: be.pairing_product(curve, P[:n], Q[:n]))
            res[f"{name}_pairing_product_{n}_pairs_per_s"] = n / t
            print(f"{name} pairing_product n={n}: {t * 1e3:.2f} ms, {n / t:,.0f} pairs/s", flush=True)
        circ = Circuit(curve, 1)
        keys = Groth16Keys(be, circ, seed=0xBE4C)
        pub = circ.arrays()["assignment"][1:2]
        proofs = keys.prove_many(list(range(max(batch_sizes))))
        for m in batch_sizes:
            pubs = np.tile(pub[None], (m, 1, 1))
            ok = keys.verify_batch(proofs[:m], pubs)
            assert ok
            t = timed(lambda: keys.verify_batch(proofs[:m], pubs))
            res[f"{name}_verify_batch_{m}_proofs_per_s"] = m / t
            print(f"{name} verify_batch count={m}: {t * 1e3:.2f} ms, {m / t:,.0f} proofs/s", flush=True)
        t0 = time.perf_counter()
        assert all(keys.verify(p, pub) for p in proofs[:64])
        th = (time.perf_counter() - t0) / 64
        res[f"{name}_host_verify_proofs_per_s"] = 1 / th
        print(f"{name} host verify loop (64 proofs): {th * 1e3:.2f} ms per proof, {1 / th:,.0f} proofs/s", flush=True)
        if not args.quick:
            res[f"{name}_speedup_1024"] = res[f"{name}_verify_batch_1024_proofs_per_s"] * th
            print(f"{name} verify_batch(1024) / host verify: {res[f'{name}_speedup_1024']:.1f}x", flush=True)
        keys.close()
    be.close()
    print(json.dumps({"pairing_bench": {k: round(v, 1) for k, v in res.items()}}), flush=True)


if __name__ == "__main__":
    main()
