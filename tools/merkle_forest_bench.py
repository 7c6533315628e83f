"""Appends into a device Merkle forest against what a caller can do without it, both curves.

  python tools/merkle_forest_bench.py [--quick] [--out profiles/merkle_forest_bench.log]

  forest    256 trees of depth 20 (capacity 2^17 leaves each) holding 2^10 resp. 2^16 leaves; one append brings 1, 16 or 1 024 leaves to EVERY tree:
            (dev) zl_merkle_forest_append_dev, leaves in device memory; (hostptr) zl_merkle_forest_append, host leaves, copies included.
  single    one tree of depth 24 (capacity 2^24) holding 2^23 leaves; 2^10 resp. 2^20 leaves appended (dev only: the capacity has room for six such appends).
  baseline  (rebuild) the parent commit's only way to a node array: zl_poseidon_merkle_build_dev once per touched tree over its full leaf set (the leaves it
            held plus the append's), device leaves, into one reused node buffer -- collecting the leaf set is not charged to it.
Every configuration starts from a fresh forest; the first append is checked before anything is timed: the forest's roots of the first, second and last tree
equal zl_poseidon_merkle_build_dev's root over those trees' leaves.  The legs are interleaved in one process, five repetitions after one warm-up round; a line
gives the median, [min .. max], leaves/s at the median and the speedup on the WORST pairing (slowest append against the fastest rebuild).  The trees grow by the
appended leaves from repetition to repetition: an append's dirty ranges depend on its size, not on the length it lands on; the rebuild stays at the first
repetition's length, the shortest it will see."""
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

from openzl_amd import ZL_BLS12_381, ZL_BN254, Backend, MerkleForest  # noqa: E402

NAMES = {ZL_BLS12_381: "bls12_381", ZL_BN254: "bn254"}
REPS = 5
LOG = []


def say(line):
    print(line, flush=True)
    LOG.append(line)


def dev_elems(n, seed):
    """n field elements below 2^251 (< r on both curves) in device memory, as an (n, 4) int64 tensor"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.randint(0, 1 << 62, (n, 4), dtype=torch.int64, device="cuda", generator=g)
    t[:, 3] &= (1 << 59) - 1
    torch.cuda.synchronize()
    return t


def interleaved(legs, reps=REPS):
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


def config(be, curve, trees, depth, capacity, base, k, host_leg, res):
    """one configuration: `trees` trees holding `base` leaves each, appends of k leaves per tree"""
    name = NAMES[curve]
    with MerkleForest(be, curve, trees, depth, capacity) as forest:
        init = dev_elems(trees * base, 11 + base % 97)
        forest.append_dev(np.repeat(np.arange(trees, dtype=np.uint32), base), init.data_ptr(), trees * base)  # tree t holds init[t * base : (t + 1) * base]
        app = dev_elems(trees * k, 13 + k)
        tree_of = np.tile(np.arange(trees, dtype=np.uint32), k)  # leaf i goes to tree i mod trees: tree t receives app[t::trees]
        app_host = app.cpu().numpy().view(np.uint64)
        n_full = base + k
        d_nodes = torch.zeros((be.L.zl_poseidon_merkle_nodes(n_full, depth), 4), dtype=torch.int64, device="cuda")
        d_full = torch.empty((n_full, 4), dtype=torch.int64, device="cuda")
        forest.append_dev(tree_of, app.data_ptr(), trees * k)  # the checked append
        roots = forest.roots()
        for t in sorted({0, min(1, trees - 1), trees - 1}):
            d_full[:base] = init[t * base:(t + 1) * base]
            d_full[base:] = app[t::trees]
            torch.cuda.synchronize()
            assert np.array_equal(be.poseidon_merkle_build_dev(curve, d_full.data_ptr(), n_full, depth, d_nodes.data_ptr()), roots[t]), (name, base, k, t)

        def rebuild():
            for _ in range(trees):
                be.poseidon_merkle_build_dev(curve, d_full.data_ptr(), n_full, depth, d_nodes.data_ptr())

        legs = {"dev": lambda: forest.append_dev(tree_of, app.data_ptr(), trees * k)}
        if host_leg:
            legs["hostptr"] = lambda: forest.append(tree_of, app_host)
        legs["rebuild"] = rebuild
        ts = interleaved(legs)
    row = {"curve": name, "trees": trees, "depth": depth, "held": base, "appended_per_tree": k}
    say(f"{name:9s} {trees:4d} trees depth {depth} holding 2^{base.bit_length() - 1:<2d} + {k:7d} leaves per tree")
    for leg, v in ts.items():
        med = statistics.median(v)
        row[leg + "_ms"] = med * 1e3
        row[leg + "_leaves_per_s"] = trees * k / med
        line = f"    {leg:8s} {fmt(v)}  {trees * k / med:14.0f} leaves/s"
        if leg != "rebuild":
            row[leg + "_worst_speedup_vs_rebuild"] = min(ts["rebuild"]) / max(v)
            line += f"   worst pairing {min(ts['rebuild']) / max(v):8.2f}x the rebuild"
        say(line)
    res.append(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="16 trees holding 2^10 leaves, no single tree: a minute's sanity run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.init()
    os.environ["ZL_TUNE_POSEIDON_DEV_MIN"] = "0"
    be = Backend(0)
    res = []
    say(f"# merkle_forest_bench: {torch.cuda.get_device_name(0)}, {REPS} repetitions after one warm-up round, legs interleaved")
    for curve in (ZL_BLS12_381, ZL_BN254):
        for base in ((1 << 10,) if args.quick else (1 << 10, 1 << 16)):
            for k in (1, 16, 1024):
                config(be, curve, 16 if args.quick else 256, 20, 1 << 17, base, k, True, res)
        if not args.quick:
            for k in (1 << 10, 1 << 20):
                config(be, curve, 1, 24, 1 << 24, 1 << 23, k, False, res)
    say("JSON " + json.dumps(res))
    be.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LOG) + "\n")


if __name__ == "__main__":
    main()
