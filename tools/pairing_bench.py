"""Throughput of the device product of pairings and of batched Groth16 verification.

  python tools/pairing_bench.py [--quick] [--decode | --decode-only] [--fexp-only]

Times zl_pairing_product at 2^10 / 2^14 / 2^16 pairs (pairs/s), Groth16Keys.verify_batch over 64 / 1 024 / 16 384 proofs of the 235-constraint Poseidon
circuit (proofs/s, OS-drawn combination as in production), and the host Groth16::verify loop over the first 64 of those proofs, on both curves.  Each
figure is the median of three timed calls after one warm-up call.  Prints one line per measurement and a JSON summary line.

--decode adds the wire-proof leg (--decode-only runs nothing else), at the same three batch sizes on both curves, over proof_to_bytes records of those proofs:
  (a) zl_groth16_proofs_from_bytes_batch (device decoder)      (b) the host loop of zl_groth16_proof_from_bytes over the same bytes
  (c) zl_groth16_verify_batch_bytes (device decode + verify)   (d) (b) followed by zl_groth16_verify_batch
(a) and (c): median of three calls after a warm-up call.  (b) and (d) are timed together (every pass of (d) contains one of (b)): median of three passes,
one pass at 16 384 proofs (half a minute of single-threaded host work per pass).

--fexp-only runs the legs of the device final exponentiation (k_pd_fexp) alone, on both curves, the two sides of every leg interleaved in one process, five
repetitions after one warm-up pair; a line gives the medians, [min .. max], their ratio and the WORST pairing of repetitions (slowest device run against
fastest host run):
  reject    Groth16Keys.verify_batch(each=True) over a batch with ONE tampered proof (a wrong public input, in the middle), at every power of two from 1 to
            16 384 proofs: (a) device final exponentiations (ZL_TUNE_FEXP_DEV_MIN=1) against (b) the host threads, the parent's code (ZL_TUNE_FEXP_DEV_MIN
            very large).  The batch is 1 024 distinct proofs repeated: the work per proof does not depend on the proofs being distinct.  Ends with T, the
            smallest power of two from which (a) beat (b) in every repetition at every size up to 16 384.
  products  Backend.pairing_products at pairs_each = 2 and 64 / 1 024 / 16 384 products against a loop of Backend.pairing_product, one call per product.  The
            loop is timed over the first 256 products and scaled to the count: its calls are independent and equal, and 16 384 of them take minutes."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openzl_amd import ZL_BLS12_381, ZL_BN254, ZL_G1, ZL_G2, Backend, Circuit, Groth16Keys  # noqa: E402
from openzl_amd.backend import G16ProofC, proof_to_bytes  # noqa: E402

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


def host_decode_loop(L, curve, data: bytes, m: int):
    """zl_groth16_proof_from_bytes record by record, as a caller without the batch entry point does it"""
    nbytes = len(data) // m
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    base = C.addressof(buf)
    out = (G16ProofC * m)()
    u8p = C.POINTER(C.c_uint8)
    for i in range(m):
        rc = L.zl_groth16_proof_from_bytes(curve, C.cast(base + i * nbytes, u8p), nbytes, C.byref(out[i]))
        assert rc == 0
    return out


def decode_leg(be, keys, curve, name, proofs, pub, batch_sizes, res):
    """every leg at the C ABI (struct arrays and byte buffers made once, outside the timed calls): the Python wrappers' per-proof tuples would be most of (a)"""
    L = be.L
    u64p = C.POINTER(C.c_uint64)
    for m in batch_sizes:
        data = b"".join(proof_to_bytes(curve, p) for p in proofs[:m])
        tuples, st = be.proofs_from_bytes(curve, data, m)
        assert not st.any() and all(np.array_equal(x, y) for p, q in zip(tuples[:64], proofs[:64]) for x, y in zip(p, q))
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        pubs = np.ascontiguousarray(np.tile(pub[None], (m, 1, 1)).reshape(-1), dtype=np.uint64)
        pp, n_public = pubs.ctypes.data_as(u64p), pub.shape[0]
        out = (G16ProofC * m)()
        status = (C.c_int32 * m)()
        ok = C.c_int(0)

        def dev_decode():
            assert L.zl_groth16_proofs_from_bytes_batch(be._ctx, curve, buf, m, out, status) == 0

        def dev_verify_bytes():
            assert L.zl_groth16_verify_batch_bytes(be._ctx, keys._k, pp, n_public, buf, m, None, C.byref(ok), None, None) == 0 and ok.value == 1

        ta = timed(dev_decode)
        assert not any(status)
        tc = timed(dev_verify_bytes)
        tb, td = [], []
        for _ in range(3 if m <= 1024 else 1):
            t0 = time.perf_counter()
            hout = host_decode_loop(L, curve, data, m)
            t1 = time.perf_counter()
            assert L.zl_groth16_verify_batch(be._ctx, keys._k, pp, n_public, hout, m, None, C.byref(ok), None) == 0 and ok.value == 1
            t2 = time.perf_counter()
            tb.append(t1 - t0)
            td.append(t2 - t0)
        tb, td = statistics.median(tb), statistics.median(td)
        for key, t, what in (("a_decode_dev", ta, "(a) proofs_from_bytes_batch"), ("b_decode_host", tb, "(b) host proof_from_bytes loop"),
                             ("c_verify_bytes", tc, "(c) verify_batch_bytes"), ("d_host_decode_verify", td, "(d) host loop + verify_batch")):
            res[f"{name}_{key}_{m}_proofs_per_s"] = m / t
            print(f"{name} {what} count={m}: {t * 1e3:.2f} ms, {m / t:,.0f} proofs/s", flush=True)
        print(f"{name} count={m}: (a) / (b) = {tb / ta:.1f}x, (c) / (d) = {td / tc:.1f}x", flush=True)


def interleaved(fa, fb, reps=5):
    """(times of fa, times of fb), the two alternating in one process after one warm-up call of each"""
    fa()
    fb()
    ta, tb = [], []
    for _ in range(reps):
        t = time.perf_counter()
        fa()
        ta.append(time.perf_counter() - t)
        t = time.perf_counter()
        fb()
        tb.append(time.perf_counter() - t)
    return ta, tb


def report(label, ta, tb, scale_b=1.0):
    tb = [t * scale_b for t in tb]
    ma, mb = statistics.median(ta), statistics.median(tb)
    worst = min(tb) / max(ta)
    print(f"{label}: (a) {ma * 1e3:.2f} ms [{min(ta) * 1e3:.2f} .. {max(ta) * 1e3:.2f}] | (b) {mb * 1e3:.2f} ms [{min(tb) * 1e3:.2f} .. {max(tb) * 1e3:.2f}]"
          f" | (b) / (a) = {mb / ma:.2f}x, worst pairing {worst:.2f}x", flush=True)
    return ma, mb, worst


def with_dev_min(value, fn):
    old = os.environ.get("ZL_TUNE_FEXP_DEV_MIN")
    os.environ["ZL_TUNE_FEXP_DEV_MIN"] = str(value)
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["ZL_TUNE_FEXP_DEV_MIN"]
        else:
            os.environ["ZL_TUNE_FEXP_DEV_MIN"] = old


def fexp_leg(be, curve, name, quick, res):
    sizes = [1, 64] if quick else [1 << k for k in range(15)]
    circ = Circuit(curve, 1)
    keys = Groth16Keys(be, circ, seed=0xBE4C)
    pub = circ.arrays()["assignment"][1:2]
    distinct = keys.prove_many(list(range(min(max(sizes), 1024))))
    wins = {}
    for m in sizes:
        proofs = [distinct[i % len(distinct)] for i in range(m)]
        pubs = np.tile(pub[None], (m, 1, 1))
        pubs[m // 2, 0, 0] ^= np.uint64(1)
        expect = np.ones(m, dtype=bool)
        expect[m // 2] = False

        def run(dev_min):
            ok, each = with_dev_min(dev_min, lambda: keys.verify_batch(proofs, pubs, each=True))
            assert not ok and (each == expect).all()

        ta, tb = interleaved(lambda: run(1), lambda: run(1 << 30))
        ma, mb, worst = report(f"{name} reject count={m}", ta, tb)
        res[f"{name}_reject_{m}_dev_ms"], res[f"{name}_reject_{m}_host_ms"], res[f"{name}_reject_{m}_worst"] = ma * 1e3, mb * 1e3, worst
        wins[m] = worst > 1.0
    t_min = None
    for m in reversed(sizes):
        if not wins[m]:
            break
        t_min = m
    res[f"{name}_T"] = float(t_min or 0)
    print(f"{name} T (smallest power of two from which the device path won every repetition): {t_min if t_min else 'none: the device path lost at the largest size'}", flush=True)
    keys.close()
    nmax = 64 if quick else 16384
    h1 = be.bases_generate(curve, scalars(curve, 2 * nmax, 5), group=ZL_G1)
    h2 = be.bases_generate(curve, scalars(curve, 2 * nmax, 6), group=ZL_G2)
    P, Q = be.bases_download(h1), be.bases_download(h2)
    be.bases_free(h1)
    be.bases_free(h2)
    for count in ([64] if quick else [64, 1024, 16384]):
        loop = min(count, 256)
        got, st = be.pairing_products(curve, P[:2 * count], Q[:2 * count], 2)
        assert not st.any() and all((got[j] == be.pairing_product(curve, P[2 * j:2 * j + 2], Q[2 * j:2 * j + 2])).all() for j in (0, count - 1))

        def single_loop():
            for j in range(loop):
                be.pairing_product(curve, P[2 * j:2 * j + 2], Q[2 * j:2 * j + 2])

        ta, tb = interleaved(lambda: be.pairing_products(curve, P[:2 * count], Q[:2 * count], 2), single_loop)
        ma, mb, worst = report(f"{name} pairing_products pairs_each=2 count={count} (loop timed over {loop} calls)", ta, tb, scale_b=count / loop)
        res[f"{name}_products_{count}_dev_ms"], res[f"{name}_products_{count}_loop_ms"], res[f"{name}_products_{count}_worst"] = ma * 1e3, mb * 1e3, worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="smallest sizes only (a smoke run of the tool)")
    ap.add_argument("--decode", action="store_true", help="add the wire-proof leg: device decoder and bytes-in verifier against the host decode loop")
    ap.add_argument("--decode-only", action="store_true", help="the wire-proof leg alone")
    ap.add_argument("--fexp-only", action="store_true", help="the legs of the device final exponentiation alone: rejected batches and pairing_products")
    args = ap.parse_args()
    be = Backend(0)
    print(be.describe(), flush=True)
    res = {}
    if args.fexp_only:
        for curve in (ZL_BLS12_381, ZL_BN254):
            fexp_leg(be, curve, NAMES[curve], args.quick, res)
        be.close()
        print(json.dumps({"pairing_bench": {k: round(v, 2) for k, v in res.items()}}), flush=True)
        return
    pair_sizes = [1 << 10] if args.quick else [1 << 10, 1 << 14, 1 << 16]
    batch_sizes = [64] if args.quick else [64, 1024, 16384]
    for curve in (ZL_BLS12_381, ZL_BN254):
        name = NAMES[curve]
        def make_proofs():
            circ = Circuit(curve, 1)
            keys = Groth16Keys(be, circ, seed=0xBE4C)
            return keys, circ.arrays()["assignment"][1:2], keys.prove_many(list(range(max(batch_sizes))))

        if args.decode_only:
            keys, pub, proofs = make_proofs()
            decode_leg(be, keys, curve, name, proofs, pub, batch_sizes, res)
            keys.close()
            continue
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
        keys, pub, proofs = make_proofs()
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
        if args.decode:  # after the existing measurements, whose order and surroundings stay as they were
            decode_leg(be, keys, curve, name, proofs, pub, batch_sizes, res)
        keys.close()
    be.close()
    print(json.dumps({"pairing_bench": {k: round(v, 1) for k, v in res.items()}}), flush=True)


if __name__ == "__main__":
    main()
