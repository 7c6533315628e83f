"""Poseidon-chain inputs in, Groth16 proofs out: the fused device call against what a caller did before it.

  python tools/chain_prove_bench.py [--quick] [--trace-only | --prove-only]

Prover leg, both curves, chains of k = 1 (235 constraints) at 64 / 256 / 1 024 / 16 384 proofs and k = 8 (1 873) at 64 / 256 / 1 024, distinct inputs per proof:
  (a)  a Python loop of witness-only Circuits (one R1CS compiler per proof, one thread), their assignments stacked, then Groth16Keys.prove_batch
  (a') the same witnesses at the C level over 16 host threads: the batch cut into 16 slices, one caller thread per slice, each calling
       zl_poseidon_chain_assignments on its HOST path (null ctx) into its rows of one array (the library's own pool of at most six workers helps
       whichever caller has blocks left), then prove_batch
  (b)  Groth16Keys.prove_chains: the trace kernel writes the assignments into the batch's block, nothing but inputs and proofs crosses the bus
over one key, interleaved in one process (a) (a') (b) (a) ..., five timed calls each after one warm-up call each; the batched prover is on its device path in
every leg (ZL_TUNE_G16_BATCH_LOG_N / _MIN set).  A line gives the median and min .. max per leg, proofs/s from the median, and for (a) / (b) and (a') / (b) the
ratio of the medians and the WORST pairing of repetitions (min of the old over max of the new).  The proofs of (b) are compared with those of (a) first.

Trace leg, both curves, k = 1, 2^10 .. 2^16 chains with inputs and rows resident on the device: zl_poseidon_chain_assignments_dev alone, seven timed calls
after a warm-up; elements/s and the effective write rate (238 x 32 bytes per chain) from the median.
Prints one line per measurement and a JSON summary line."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the backend: torch initialises its HIP runtime first, as in bench.py)

from openzl_amd import ZL_BLS12_381, ZL_BN254, Backend, Circuit, Groth16Keys, load_library, poseidon_chain_assignment_elems, poseidon_chain_assignments_host  # noqa: E402
from openzl_amd.backend import _p64  # noqa: E402

NAMES = {ZL_BLS12_381: "bls12_381", ZL_BN254: "bn254"}
HOST_THREADS = 16
_EX = ThreadPoolExecutor(max_workers=HOST_THREADS)


def assignments_16_threads(curve, x0, x1, k):
    """(count, nv, 4) assignments: 16 caller threads, one contiguous slice each, through the host path of zl_poseidon_chain_assignments (ctypes drops the GIL)"""
    L = load_library()
    n = x0.shape[0]
    out = np.empty((n, poseidon_chain_assignment_elems(k), 4), dtype=np.uint64)
    cuts = [n * i // HOST_THREADS for i in range(HOST_THREADS + 1)]

    def part(i):
        lo, hi = cuts[i], cuts[i + 1]
        if hi > lo:
            rc = L.zl_poseidon_chain_assignments(None, curve, _p64(x0[lo:hi]), _p64(x1[lo:hi]), k, hi - lo, _p64(out[lo:hi]))
            assert rc == 0, rc

    list(_EX.map(part, range(HOST_THREADS)))
    return out


def scalars(n, seed):
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 2 ** 63, size=(n, 4), dtype=np.uint64)
    out[:, 3] &= np.uint64((1 << 59) - 1)  # < 2^251 < r of both curves
    return out


def as_int(row) -> int:
    return sum(int(v) << (64 * j) for j, v in enumerate(row))


def interleaved(fns, reps):
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, ts):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
    return ts


def same(p, q):
    return all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(p, q))


def prove_leg(be, res, quick):
    os.environ["ZL_TUNE_G16_BATCH_LOG_N"] = "28"
    os.environ["ZL_TUNE_G16_BATCH_MIN"] = "1"
    shapes = [(1, [64])] if quick else [(1, [64, 256, 1024, 16384]), (8, [64, 256, 1024])]
    for curve in (ZL_BLS12_381, ZL_BN254):
        for k, counts in shapes:
            circ = Circuit(curve, k)
            keys = Groth16Keys(be, circ, seed=0xC4A1)
            nc = circ.shape[0]
            name = f"{NAMES[curve]} k={k} ({nc} constraints)"
            for count in counts:
                x0, x1 = scalars(count, 41 + count), scalars(count, 42 + count)
                x0i, x1i = [as_int(v) for v in x0], [as_int(v) for v in x1]
                r, s = scalars(count, 31 + count), scalars(count, 32 + count)

                def loop_of_circuits():
                    zs = []
                    for a, b in zip(x0i, x1i):
                        c = Circuit(curve, k, x0=a, x1=b, witness_only=True)
                        zs.append(c.arrays()["assignment"])
                        c.close()
                    return keys.prove_batch(np.stack(zs), r, s)

                def host_pool():
                    return keys.prove_batch(assignments_16_threads(curve, x0, x1, k), r, s)

                def fused():
                    return keys.prove_chains(x0, x1, r, s)[0]

                assert np.array_equal(assignments_16_threads(curve, x0, x1, k), poseidon_chain_assignments_host(curve, x0, x1, k)), name
                ref, got = loop_of_circuits(), fused()
                assert len(got) == count and all(same(g, e) for g, e in zip(got, ref)), name
                assert all(same(g, e) for g, e in zip(host_pool()[:4], ref[:4])), name
                ta, tp, tb = interleaved([loop_of_circuits, host_pool, fused], 5)
                ma, mp, mb = (statistics.median(t) for t in (ta, tp, tb))
                key = f"{NAMES[curve]}_k{k}_count{count}"
                res[key + "_loop_per_s"], res[key + "_threads16_per_s"], res[key + "_fused_per_s"] = count / ma, count / mp, count / mb
                res[key + "_loop_over_fused_worst"], res[key + "_threads16_over_fused_worst"] = min(ta) / max(tb), min(tp) / max(tb)
                fmt = lambda t: f"{statistics.median(t) * 1e3:.2f} ms [{min(t) * 1e3:.2f} .. {max(t) * 1e3:.2f}], {count / statistics.median(t):,.0f} proofs/s"  # noqa: E731
                print(f"{name} count={count}: (a) {fmt(ta)} | (a') {fmt(tp)} | (b) {fmt(tb)} | (a) / (b) = {ma / mb:.2f}x, worst pairing {min(ta) / max(tb):.2f}x | "
                      f"(a') / (b) = {mp / mb:.2f}x, worst pairing {min(tp) / max(tb):.2f}x", flush=True)
            keys.close()
            circ.close()
    del os.environ["ZL_TUNE_G16_BATCH_LOG_N"], os.environ["ZL_TUNE_G16_BATCH_MIN"]


def trace_leg(be, res, quick):
    k = 1
    nv = poseidon_chain_assignment_elems(k)
    logs = [10] if quick else list(range(10, 17))
    for curve in (ZL_BLS12_381, ZL_BN254):
        n_max = 1 << max(logs)
        d0 = torch.from_numpy(scalars(n_max, 51).view(np.int64)).cuda()
        d1 = torch.from_numpy(scalars(n_max, 52).view(np.int64)).cuda()
        d_out = torch.zeros(n_max * nv * 4, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        exp = poseidon_chain_assignments_host(curve, scalars(n_max, 51)[:3], scalars(n_max, 52)[:3], k)
        for lg in logs:
            n = 1 << lg
            run = lambda: be.poseidon_chain_assignments_dev(curve, d0.data_ptr(), d1.data_ptr(), k, n, d_out.data_ptr())  # noqa: E731  (finished on return)
            (ts,) = interleaved([run], 7)
            assert np.array_equal(d_out[: 3 * nv * 4].cpu().numpy().view(np.uint64).reshape(3, nv, 4), exp)
            m = statistics.median(ts)
            res[f"{NAMES[curve]}_trace_2^{lg}_elems_per_s"] = n * nv / m
            print(f"{NAMES[curve]} trace k={k} chains=2^{lg}: {m * 1e3:.3f} ms [{min(ts) * 1e3:.3f} .. {max(ts) * 1e3:.3f}], {n / m:,.0f} chains/s, "
                  f"{n * nv / m:,.0f} elements/s, {n * nv * 32 / m / 1e9:.2f} GB/s written", flush=True)
        del d0, d1, d_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="smallest shape only (a smoke run of the tool)")
    ap.add_argument("--trace-only", action="store_true", help="the trace-kernel leg alone")
    ap.add_argument("--prove-only", action="store_true", help="the prover leg alone")
    args = ap.parse_args()
    if torch.cuda.is_available():
        torch.cuda.init()
    be = Backend(0)
    print(be.describe(), flush=True)
    res = {}
    if not args.prove_only:
        trace_leg(be, res, args.quick)
    if not args.trace_only:
        prove_leg(be, res, args.quick)
    be.close()
    print(json.dumps({"chain_prove_bench": {k: round(v, 2) for k, v in res.items()}}), flush=True)


if __name__ == "__main__":
    main()
