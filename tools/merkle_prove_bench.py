"""Merkle memberships in, Groth16 proofs out: the fused device calls against what a caller can write with the circuit alone.

  python tools/merkle_prove_bench.py [--quick] [--trace-only | --prove-only] [--depths 4,8,20] [--counts 64,1024,16384] [--reps 5]

Prover leg, both curves, depth 4 (949 constraints, domain 2^10), 8 (1 897, 2^11) and 20 (4 741, 2^13) at 64 / 1 024 / 16 384 memberships of one tree
(min(2^depth, 2^16) leaves, built on the device; the leaf indices are drawn at random, the paths gathered once, outside the timed calls), DEFAULT dispatch --
no tuning variable is set, so depth 20 loops the resident prover in every leg:
  (a) a Python loop of witness-only Circuit.merkle compilers (one per proof, one thread), their assignments stacked, then Groth16Keys.prove_batch
  (b) Groth16Keys.prove_merkle_paths: leaves, indices and paths go up, the trace kernel writes the assignments into the batch's block
  (c) Groth16Keys.prove_merkle_members: only the indices go up, leaf and siblings are read out of the node array
over one key, interleaved in one process (a) (b) (c) (a) ..., `reps` timed calls each after one warm-up call each.  A line gives the median and min .. max per
leg, proofs/s from the median, and for (a) / (b) and (a) / (c) the ratio of the medians and the WORST pairing of repetitions (min of the old over max of the
new).  The proofs of (b) and (c) are compared with those of (a) first.

Trace leg, both curves, depth 8, 2^10 .. 2^16 rows with leaves, paths, the tree and the rows resident on the device (the indices are host memory by the
interface): zl_poseidon_merkle_assignments_dev and zl_poseidon_merkle_member_assignments_dev alone, seven timed calls after a warm-up; rows/s and the effective
write rate (1 907 x 32 bytes per row) from the median.
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

from openzl_amd import (ZL_BLS12_381, ZL_BN254, Backend, Circuit, Groth16Keys, poseidon_merkle_assignment_elems, poseidon_merkle_assignments_host,  # noqa: E402
                        poseidon_merkle_nodes)

NAMES = {ZL_BLS12_381: "bls12_381", ZL_BN254: "bn254"}


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


def device_tree(be, curve, depth, seed):
    """(the node array on the device, n, the leaves on the host): min(2^depth, 2^16) random leaves"""
    n = min(1 << depth, 1 << 16)
    leaves = scalars(n, seed)
    d_leaves = torch.from_numpy(leaves.view(np.int64)).cuda()
    d_nodes = torch.zeros(poseidon_merkle_nodes(n, depth) * 4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    be.poseidon_merkle_build_dev(curve, d_leaves.data_ptr(), n, depth, d_nodes.data_ptr())
    return d_nodes, n, leaves


def prove_leg(be, res, depths, counts, reps):
    for name in ("ZL_TUNE_G16_BATCH_LOG_N", "ZL_TUNE_G16_BATCH_MIN", "ZL_TUNE_POSEIDON_DEV_MIN"):
        assert name not in os.environ, name + " is set: this leg measures the default dispatch"
    for curve in (ZL_BLS12_381, ZL_BN254):
        for depth in depths:
            circ = Circuit.merkle(curve, depth, 1, 0, [2] * depth)
            keys = Groth16Keys(be, circ, seed=0x3E21)
            nc = circ.shape[0]
            log_n = max(1, (nc + 1).bit_length())
            name = f"{NAMES[curve]} depth={depth} ({nc} constraints, domain 2^{log_n})"
            d_nodes, n, leaves = device_tree(be, curve, depth, 60 + depth)
            for count in counts:
                ix = np.random.default_rng(61 + count).integers(0, n, size=count, dtype=np.uint64)
                lv = np.ascontiguousarray(leaves[ix.astype(np.int64)])
                paths = be.poseidon_merkle_paths(curve, d_nodes.data_ptr(), n, depth, ix)
                lvi, ixi, pai = [as_int(v) for v in lv], [int(v) for v in ix], [[as_int(v) for v in p] for p in paths]
                r, s = scalars(count, 31 + count), scalars(count, 32 + count)

                def loop_of_circuits():
                    zs = np.empty((count, poseidon_merkle_assignment_elems(depth), 4), dtype=np.uint64)
                    for j in range(count):
                        c = Circuit.merkle(curve, depth, lvi[j], ixi[j], pai[j], witness_only=True)
                        zs[j] = c.arrays()["assignment"]
                        c.close()
                    return keys.prove_batch(zs, r, s)

                def from_paths():
                    return keys.prove_merkle_paths(lv, ix, paths, r, s)[0]

                def from_tree():
                    return keys.prove_merkle_members(d_nodes.data_ptr(), n, ix, r, s)[0]

                ref, got_b, got_c = loop_of_circuits(), from_paths(), from_tree()
                assert len(got_b) == len(got_c) == count and all(same(g, e) for g, e in zip(got_b, ref)) and all(same(g, e) for g, e in zip(got_c, ref)), name
                ta, tb, tc = interleaved([loop_of_circuits, from_paths, from_tree], reps)
                ma, mb, mc = (statistics.median(t) for t in (ta, tb, tc))
                key = f"{NAMES[curve]}_d{depth}_count{count}"
                res[key + "_loop_per_s"], res[key + "_paths_per_s"], res[key + "_members_per_s"] = count / ma, count / mb, count / mc
                res[key + "_loop_over_paths_worst"], res[key + "_loop_over_members_worst"] = min(ta) / max(tb), min(ta) / max(tc)
                fmt = lambda t: f"{statistics.median(t) * 1e3:.2f} ms [{min(t) * 1e3:.2f} .. {max(t) * 1e3:.2f}], {count / statistics.median(t):,.0f} proofs/s"  # noqa: E731
                print(f"{name} count={count} reps={reps}: (a) {fmt(ta)} | (b) {fmt(tb)} | (c) {fmt(tc)} | (a) / (b) = {ma / mb:.2f}x, worst pairing "
                      f"{min(ta) / max(tb):.2f}x | (a) / (c) = {ma / mc:.2f}x, worst pairing {min(ta) / max(tc):.2f}x", flush=True)
            keys.close()
            circ.close()
            del d_nodes


def trace_leg(be, res, quick):
    depth = 8
    nv = poseidon_merkle_assignment_elems(depth)
    logs = [10] if quick else list(range(10, 17))
    for curve in (ZL_BLS12_381, ZL_BN254):
        n_max = 1 << max(logs)
        d_nodes, n, leaves = device_tree(be, curve, depth, 71)
        ix_all = np.random.default_rng(72).integers(0, n, size=n_max, dtype=np.uint64)
        lv = np.ascontiguousarray(leaves[ix_all.astype(np.int64)])
        paths = be.poseidon_merkle_paths(curve, d_nodes.data_ptr(), n, depth, ix_all)
        d_lv = torch.from_numpy(lv.view(np.int64)).cuda()
        d_pa = torch.from_numpy(paths.view(np.int64)).cuda()
        d_out = torch.zeros(n_max * nv * 4, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        exp = poseidon_merkle_assignments_host(curve, lv[:3], ix_all[:3], paths[:3], depth)
        for lg in logs:
            rows = 1 << lg
            ix = ix_all[:rows]
            from_paths = lambda: be.poseidon_merkle_assignments_dev(curve, d_lv.data_ptr(), ix, d_pa.data_ptr(), depth, d_out.data_ptr())  # noqa: E731  (finished on return)
            from_tree = lambda: be.poseidon_merkle_member_assignments_dev(curve, d_nodes.data_ptr(), n, depth, ix, d_out.data_ptr())  # noqa: E731
            for what, run in (("paths", from_paths), ("members", from_tree)):
                d_out[: 3 * nv * 4].zero_()
                (ts,) = interleaved([run], 7)
                assert np.array_equal(d_out[: 3 * nv * 4].cpu().numpy().view(np.uint64).reshape(3, nv, 4), exp)
                m = statistics.median(ts)
                res[f"{NAMES[curve]}_trace_{what}_2^{lg}_rows_per_s"] = rows / m
                print(f"{NAMES[curve]} trace depth={depth} {what} rows=2^{lg}: {m * 1e3:.3f} ms [{min(ts) * 1e3:.3f} .. {max(ts) * 1e3:.3f}], {rows / m:,.0f} rows/s, "
                      f"{rows * nv / m:,.0f} elements/s, {rows * nv * 32 / m / 1e9:.2f} GB/s written", flush=True)
        del d_lv, d_pa, d_out, d_nodes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="smallest shape only (a smoke run of the tool)")
    ap.add_argument("--trace-only", action="store_true", help="the trace-kernel leg alone")
    ap.add_argument("--prove-only", action="store_true", help="the prover leg alone")
    ap.add_argument("--depths", default="4,8,20")
    ap.add_argument("--counts", default="64,1024,16384")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    depths = [4] if args.quick else [int(v) for v in args.depths.split(",")]
    counts = [64] if args.quick else [int(v) for v in args.counts.split(",")]
    if torch.cuda.is_available():
        torch.cuda.init()
    be = Backend(0)
    print(be.describe(), flush=True)
    res = {}
    if not args.prove_only:
        trace_leg(be, res, args.quick)
    if not args.trace_only:
        prove_leg(be, res, depths, counts, args.reps)
    be.close()
    print(json.dumps({"merkle_prove_bench": {k: round(v, 2) for k, v in res.items()}}), flush=True)


if __name__ == "__main__":
    main()
