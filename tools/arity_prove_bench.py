"""The three fused provers of the arity-general circuits against what a caller writes without them, both curves.

  python tools/arity_prove_bench.py [--quick] [--counts 64,1024,16384] [--resident-max N] [--out profiles/arity_prove_bench.log]

  hashes   Groth16Keys.prove_hashes at arity 3 and 5
  paths    Groth16Keys.prove_merkle_leaf_paths at (arity 4, depth 4) and (arity 4, depth 8)
  members  Groth16Keys.prove_merkle_leaf_members at the same shapes, over a full tree of 2^depth leaves hashed on the device from their preimages
  baseline (loop) one witness-only Circuit per proof -- Circuit.poseidon_hash / Circuit.merkle_leaf -- its assignment copied out, then Groth16Keys.prove_batch
           over the stacked assignments: synthesis on the host, the assignments over the bus.
Dispatch is the library's own (no ZL_TUNE_G16_* set): domains up to 2^11 with at least 64 proofs stay on the device, so (4, 8) -- domain 2^12 -- loops the resident
prover in every leg and shows what the fused call saves there: synthesis and the upload, not the batched MSMs.  Before anything is timed the fused proofs of
the first configuration are checked against the baseline's, byte for byte.  The legs are interleaved in one process, five repetitions after one warm-up round;
a line gives the median, [min .. max], proofs/s at the median and the speedup on the WORST pairing (slowest fused call against the fastest loop).

  trace    k_pos_hash_trace / k_pos_leaf_merkle_trace alone, device operands, 2^10 .. 2^16 rows: the expectation is ONE dependent permutation chain per launch
           whatever the row count -- about 0.64 / 0.96 / 1.31 ms at widths 4 / 5 / 6 plus depth x 0.53 ms for the levels -- until the rows fill the device."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (its HIP runtime initialises first, as in bench.py)

from openzl_amd import ZL_BLS12_381, ZL_BN254, Backend, Circuit, Groth16Keys, poseidon_merkle_nodes  # noqa: E402

NAMES = {ZL_BLS12_381: "bls12_381", ZL_BN254: "bn254"}
REPS = 5
LOG = []


def say(line):
    print(line, flush=True)
    LOG.append(line)


def elems(n, seed):
    """n field elements below 2^251 (< r on both curves) as an (n, 4) uint64 array"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 59) - 1)
    return a


def ints(a):
    return [sum(int(w) << (64 * j) for j, w in enumerate(row)) for row in np.asarray(a).reshape(-1, 4)]


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def interleaved(legs, reps):
    for fn in legs.values():
        fn()
    ts = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            t = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t)
    return ts


def fmt(ts):
    v = [t * 1e3 for t in ts]
    return f"{statistics.median(v):10.3f} ms [{min(v):.3f} .. {max(v):.3f}]"


def same(p, q):
    return all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(p, q))


def report(name, what, count, ts, res, row):
    say(f"{name:9s} {what}  {count:6d} proofs")
    for leg, v in ts.items():
        med = statistics.median(v)
        row[leg + "_ms"] = med * 1e3
        line = f"    {leg:8s} {fmt(v)}  {count / med:12.0f} proofs/s"
        if leg != "loop":
            row[leg + "_worst_speedup_vs_loop"] = min(ts["loop"]) / max(v)
            line += f"   worst pairing {min(ts['loop']) / max(v):7.2f}x the loop"
        say(line)
    res.append(row)


def loop_assignments(make, count):
    rows = []
    for j in range(count):
        w = make(j)
        rows.append(w.arrays()["assignment"])
        w.close()
    return np.stack(rows)


def hashes(be, curve, arity, counts, reps, res, check):
    name = NAMES[curve]
    top = max(counts)
    v = elems(top * arity, 31 + arity).reshape(top, arity, 4)
    xs = [ints(row) for row in v]
    r, s = elems(top, 32), elems(top, 33)
    full = Circuit.poseidon_hash(curve, xs[0])
    keys = Groth16Keys(be, full, seed=41)

    def loop(c):
        return keys.prove_batch(loop_assignments(lambda j: Circuit.poseidon_hash(curve, xs[j], witness_only=True), c), r[:c], s[:c])

    if check:
        got, _ = keys.prove_hashes(v[:70], r[:70], s[:70])
        assert all(same(a, b) for a, b in zip(got, loop(70))), "fused proofs differ from the loop's"
    for c in counts:
        ts = interleaved({"fused": lambda: keys.prove_hashes(v[:c], r[:c], s[:c]), "loop": lambda: loop(c)}, reps)
        report(name, f"hash arity {arity}          ", c, ts, res, {"curve": name, "circuit": "hash", "arity": arity, "count": c})
    keys.close()
    full.close()


def leaves(be, curve, arity, depth, counts, reps, res, check, resident_max):
    name = NAMES[curve]
    if resident_max and 285 + 237 * depth + 2 > 2048:  # arity 4: a domain above 2^11 loops the resident prover in every leg, ~1.5 ms a proof
        skipped = [c for c in counts if c > resident_max]
        counts = [c for c in counts if c <= resident_max]
        if skipped:
            say(f"{name:9s} leaf arity {arity} depth {depth:2d}: counts {skipped} skipped (--resident-max {resident_max})")
    top, n = max(counts), 1 << depth
    pre = elems(n * arity, 51 + depth).reshape(n, arity, 4)
    d_pre = dev(pre)
    d_leaves = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    be.poseidon_hash_dev(curve, arity, d_pre.data_ptr(), n, d_leaves.data_ptr())
    d_nodes = torch.zeros((poseidon_merkle_nodes(n, depth), 4), dtype=torch.int64, device="cuda")
    be.poseidon_merkle_build_dev(curve, d_leaves.data_ptr(), n, depth, d_nodes.data_ptr())
    ix = np.random.default_rng(52).integers(0, n, size=top).astype(np.uint64)
    paths = be.poseidon_merkle_paths(curve, d_nodes.data_ptr(), n, depth, ix)
    pv = np.ascontiguousarray(pre[ix.astype(np.int64)])
    xs, ps = [ints(row) for row in pre], [ints(row) for row in paths]
    r, s = elems(top, 53), elems(top, 54)
    full = Circuit.merkle_leaf(curve, depth, xs[int(ix[0])], int(ix[0]), ps[0])
    keys = Groth16Keys(be, full, seed=43)

    def loop(c):
        return keys.prove_batch(loop_assignments(lambda j: Circuit.merkle_leaf(curve, depth, xs[int(ix[j])], int(ix[j]), ps[j], witness_only=True), c), r[:c], s[:c])

    if check:
        exp = loop(70)
        for got, _ in (keys.prove_merkle_leaf_paths(pv[:70], ix[:70], paths[:70], r[:70], s[:70]),
                       keys.prove_merkle_leaf_members(d_nodes.data_ptr(), d_pre.data_ptr(), n, ix[:70], r[:70], s[:70])):
            assert all(same(a, b) for a, b in zip(got, exp)), "fused proofs differ from the loop's"
    for c in counts:
        legs = {"paths": lambda: keys.prove_merkle_leaf_paths(pv[:c], ix[:c], paths[:c], r[:c], s[:c]),
                "members": lambda: keys.prove_merkle_leaf_members(d_nodes.data_ptr(), d_pre.data_ptr(), n, ix[:c], r[:c], s[:c]), "loop": lambda: loop(c)}
        ts = interleaved(legs, reps)
        report(name, f"leaf arity {arity} depth {depth:2d}", c, ts, res, {"curve": name, "circuit": "leaf", "arity": arity, "depth": depth, "count": c})
    keys.close()
    full.close()


def traces(be, curve, logs, reps, res):
    """the trace kernels alone: device operands in, dense rows out"""
    name = NAMES[curve]
    for log in logs:
        n = 1 << log
        row = {"curve": name, "circuit": "trace", "rows": n}
        line = f"{name:9s} trace 2^{log:<2d} rows:"
        for arity, depth in ((3, 0), (4, 0), (5, 0), (4, 4), (4, 8)):
            d_in = dev(elems(n * arity, 61 + log))
            nv = be.L.zl_poseidon_merkle_leaf_assignment_elems(arity, depth) if depth else be.L.zl_poseidon_hash_assignment_elems(arity)
            d_out = torch.empty((n, nv, 4), dtype=torch.int64, device="cuda")
            if depth:
                d_pa = dev(elems(n * depth, 62 + log))
                ix = np.random.default_rng(63).integers(0, 1 << depth, size=n).astype(np.uint64)
                fn = lambda: be.poseidon_merkle_leaf_assignments_dev(curve, arity, d_in.data_ptr(), ix, d_pa.data_ptr(), depth, d_out.data_ptr())  # noqa: E731
            else:
                fn = lambda: be.poseidon_hash_assignments_dev(curve, arity, d_in.data_ptr(), n, d_out.data_ptr())  # noqa: E731
            ts = interleaved({"t": fn}, reps)["t"]
            tag = f"a{arity}" + (f"d{depth}" if depth else "")
            row[tag + "_ms"] = statistics.median(ts) * 1e3
            row[tag + "_max_ms"] = max(ts) * 1e3
            line += f"  {tag} {statistics.median(ts) * 1e3:7.3f} (max {max(ts) * 1e3:.3f})"
            del d_out
        say(line + " ms")
        res.append(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="counts 64 and 1024, traces at 2^10 and 2^14: a few minutes")
    ap.add_argument("--counts", default=None, help="comma-separated proof counts (default 64,1024,16384)")
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--resident-max", type=int, default=0, help="largest count run for a shape whose domain is above 2^11 (every leg loops the resident prover); 0 = all")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    counts = [int(c) for c in args.counts.split(",")] if args.counts else ([64, 1024] if args.quick else [64, 1024, 16384])
    torch.cuda.init()
    for k in ("ZL_TUNE_G16_BATCH_LOG_N", "ZL_TUNE_G16_BATCH_MIN", "ZL_TUNE_G16_BATCH_CHUNK", "ZL_TUNE_POSEIDON_DEV_MIN", "ZL_TUNE_POSEIDON_CHUNK"):
        os.environ.pop(k, None)
    be = Backend(0)
    res = []
    say(f"# arity_prove_bench: {torch.cuda.get_device_name(0)}, {args.reps} repetitions after one warm-up round, legs interleaved, counts {counts}")
    for curve in (ZL_BLS12_381, ZL_BN254):
        for i, arity in enumerate((3, 5)):
            hashes(be, curve, arity, counts, args.reps, res, i == 0)
        for i, depth in enumerate((4, 8)):
            leaves(be, curve, 4, depth, counts, args.reps, res, i == 0, args.resident_max)
        traces(be, curve, (10, 14) if args.quick else (10, 12, 14, 16), args.reps, res)
    say("JSON " + json.dumps(res))
    be.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LOG) + "\n")


if __name__ == "__main__":
    main()
