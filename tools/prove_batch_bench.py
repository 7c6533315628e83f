"""Throughput of the batched Groth16 prover and of the multi-vector MSM under it.

  python tools/prove_batch_bench.py [--quick] [--msm-only | --prove-only]

Prover leg, both curves, Poseidon hash chains of 235 / 1 882 / 14 977 constraints (k = 1 / 8 / 64), count = 64 / 1 024 (and 16 384 at 235 constraints):
  (a) zl_groth16_prove_batch on its device path (ZL_TUNE_G16_BATCH_LOG_N / _MIN set so that every shape takes it)
  (b) zl_groth16_prove_circuits, the unchanged two-lane stream (Groth16Keys.prove_many)
over the same key and witness, interleaved in one process (a) (b) (a) (b) ..., three timed calls each after one warm-up call each.  A line gives the median
and min .. max of the per-call times, proofs/s from the median, the ratio (b) / (a) of the medians and the smallest ratio any pairing of repetitions gives
(min of (b) over max of (a)): the device path is made the default only where that worst pairing exceeds the +-4 % between boxes.  The first proofs of (a) are
compared with zl_groth16_prove_resident before anything is timed.

MSM leg, G1 and G2 of both curves, n = 2^9 / 2^12 / 2^15 points and count = 64 / 1 024 uniform scalar vectors resident on the device:
  (a) zl_msm_multi_dev             one call, canonical affine results on the host
  (b) zl_msm_batch_partial_dev     the same vectors as `count` pipelined MSMs, un-normalised partial sums on the host (its callers still normalise them)
interleaved the same way, five timed calls each.  Result 0 of (a) is compared with the folded partial 0 of (b) before anything is timed.
Prints one line per measurement and a JSON summary line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the backend: torch initialises its HIP runtime first, as in bench.py)

from openzl_amd import ZL_BLS12_381, ZL_BN254, ZL_G1, ZL_G2, Backend, Circuit, Groth16Keys  # noqa: E402

NAMES = {ZL_BLS12_381: "bls12_381", ZL_BN254: "bn254"}


def scalars(n, seed):
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 2 ** 63, size=(n, 4), dtype=np.uint64)
    out[:, 3] &= np.uint64((1 << 59) - 1)  # < 2^251 < r of both curves
    return out


def line(name, what, unit, count, ta, tb, res, key):
    ma, mb = statistics.median(ta), statistics.median(tb)
    res[key + "_a_per_s"] = count / ma
    res[key + "_b_per_s"] = count / mb
    res[key + "_ratio"] = mb / ma
    res[key + "_ratio_worst"] = min(tb) / max(ta)
    print(f"{name} {what} count={count}: (a) {ma * 1e3:.2f} ms [{min(ta) * 1e3:.2f} .. {max(ta) * 1e3:.2f}], {count / ma:,.0f} {unit}/s | "
          f"(b) {mb * 1e3:.2f} ms [{min(tb) * 1e3:.2f} .. {max(tb) * 1e3:.2f}], {count / mb:,.0f} {unit}/s | (b) / (a) = {mb / ma:.2f}x, worst pairing {min(tb) / max(ta):.2f}x",
          flush=True)


def interleaved(fa, fb, reps):
    fa()
    fb()
    ta, tb = [], []
    for _ in range(reps):
        for fn, ts in ((fa, ta), (fb, tb)):
            t = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t)
    return ta, tb


def prove_leg(be, res, quick):
    os.environ["ZL_TUNE_G16_BATCH_LOG_N"] = "28"  # (a) is the device path at every shape; (b) does not read the knobs
    os.environ["ZL_TUNE_G16_BATCH_MIN"] = "1"
    shapes = [(1, [64])] if quick else [(1, [64, 1024, 16384]), (8, [64, 1024]), (64, [64, 1024])]
    for curve in (ZL_BLS12_381, ZL_BN254):
        for k, counts in shapes:
            circ = Circuit(curve, k)
            keys = Groth16Keys(be, circ, seed=0xBA7C)
            z = circ.arrays()["assignment"]
            nc = circ.shape[0]
            name = f"{NAMES[curve]} {nc} constraints"
            for count in counts:
                Z = np.ascontiguousarray(np.broadcast_to(z, (count,) + z.shape))
                r, s = scalars(count, 31 + count), scalars(count, 32 + count)
                seeds = list(range(count))
                got = keys.prove_batch(Z[:2], r[:2], s[:2])
                pk, hr = keys.pk_dict(), keys._r1cs
                for j in range(2):
                    ref = be.groth16_prove_resident(curve, pk, hr, Z[j], r[j], s[j])
                    assert all(np.array_equal(x, y) for x, y in zip(got[j], ref)), (name, j)
                ta, tb = interleaved(lambda: keys.prove_batch(Z, r, s), lambda: keys.prove_many(seeds), 3)
                line(name, "prove", "proofs", count, ta, tb, res, f"{NAMES[curve]}_prove_{nc}_count{count}")
            keys.close()
            circ.close()
    del os.environ["ZL_TUNE_G16_BATCH_LOG_N"], os.environ["ZL_TUNE_G16_BATCH_MIN"]


def msm_leg(be, res, quick):
    sizes = [1 << 9] if quick else [1 << 9, 1 << 12, 1 << 15]
    counts = [64] if quick else [64, 1024]
    for curve in (ZL_BLS12_381, ZL_BN254):
        for group in (ZL_G1, ZL_G2):
            name = f"{NAMES[curve]}_g{group}"
            h = be.bases_generate(curve, scalars(max(sizes), 11 * curve + group), group=group)
            for n in sizes:
                for count in counts:
                    d = torch.from_numpy(scalars(count * n, 1000 + n + count).view(np.int64)).cuda()
                    torch.cuda.synchronize()
                    ptrs = [d.data_ptr() + j * n * 32 for j in range(count)]
                    multi = lambda: be.msm_multi_dev(h, d.data_ptr(), n, count)  # noqa: E731
                    batch = lambda: be.msm_batch_partial_dev(h, ptrs, n)  # noqa: E731
                    (xy, inf), parts = multi(), batch()
                    exp, einf = be.partials_sum(curve, parts[0:1], group=group)
                    assert inf[0] == einf and (xy[0] == exp).all(), (name, n, count)
                    ta, tb = interleaved(multi, batch, 5)
                    line(name, f"msm n={n}", "MSMs", count, ta, tb, res, f"{name}_n{n}_count{count}")
                    del d
            be.bases_free(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="smallest shape only (a smoke run of the tool)")
    ap.add_argument("--msm-only", action="store_true", help="the MSM leg alone")
    ap.add_argument("--prove-only", action="store_true", help="the prover leg alone")
    args = ap.parse_args()
    if torch.cuda.is_available():
        torch.cuda.init()
    be = Backend(0)
    print(be.describe(), flush=True)
    res = {}
    if not args.msm_only:
        prove_leg(be, res, args.quick)
    if not args.prove_only:
        msm_leg(be, res, args.quick)
    be.close()
    print(json.dumps({"prove_batch_bench": {k: round(v, 2) for k, v in res.items()}}), flush=True)


if __name__ == "__main__":
    main()
