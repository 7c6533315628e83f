"""Throughput of the batched Poseidon entry points, both curves.

  python tools/poseidon_bench.py [--quick] [--out profiles/poseidon_bench.log]

Every leg is checked before it is timed, its sides are interleaved in one process, five repetitions after one warm-up round; a line gives the median,
[min .. max], and ratios on the WORST pairing of repetitions (slowest run of the new path against the fastest run of the old one).

  hash2     zl_poseidon_hash2_batch at 2^6 .. 2^22 pairs: (dev) device operands, zl_poseidon_hash2_batch_dev; (hostptr) host operands, copies included;
            (pool) the ctx == NULL host path; against the loop over zl_poseidon_permute a caller of the parent commit writes, (loop1) on one thread and
            (loopT) sliced over the granted host threads.  The loops are timed over at most 2^12 permutations and scaled (equal, independent calls); they are
            ctypes calls, about a microsecond of call overhead each.  Derived: Fr multiplications/s = 804 x permutations/s.
  devmin    host-pointer hash2 on the device against the host path at every power of two up to 2^12: the smallest count from which the device wins every
            repetition is the default of ZL_TUNE_POSEIDON_DEV_MIN.
  merkle    zl_poseidon_merkle_build_dev at 2^10 .. 2^24 leaves (depth = log2 n) with the default tail; at 2^20 leaves the tail threshold T is swept over
            0, 16, 64, 256, 1024, and the upper T-leaf tree is also built alone with and without the tail kernel (the levels above the threshold).
  fold      zl_poseidon_merkle_roots_from_paths at depth 20 for 2^10 and 2^16 paths (host operands, copies included).
  arity     (--arity: this leg alone, to profiles/poseidon_arity_bench.log) zl_poseidon_hash_batch at arities 2 .. 5 (widths 3 .. 6), 2^6 .. 2^22 items:
            (dev) device operands, (hostptr) host operands, interleaved with (hash2 dev / hash2 hostptr) the width-3 hash2 leg as the scale and (loopT) the
            loop a caller writes without the batch: zl_poseidon_permute_w sliced over the granted host threads (at most 2^12 permutations, scaled).  Up to
            2^10 items also (pool) the ctx == NULL host path: a width whose device call at 64 items loses a repetition to it needs a larger DEV_MIN.
            Derived: time per permutation against the product count of the plain schedule, 804 / 1 288 / 1 976 / 2 616.
Checks: hash2 against the zl_poseidon_permute loop (all pairs up to 2^12, a sample of 256 above); trees up to 2^16 leaves against the host path node for
node, larger ones by folding 32 gathered paths with the zl_poseidon_permute loop to the device's root; folds against the tree's root."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (its HIP runtime initialises first, as in bench.py)

from openzl_amd import ZL_BLS12_381, ZL_BN254, Backend  # noqa: E402
from openzl_amd import backend as zb  # noqa: E402

NAMES = {ZL_BLS12_381: "bls12_381", ZL_BN254: "bn254"}
REPS = 5
LOG = []


def say(line):
    print(line, flush=True)
    LOG.append(line)


def elems(n, seed):
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 2 ** 63, size=(n, 4), dtype=np.uint64)
    out[:, 3] &= np.uint64((1 << 59) - 1)  # < 2^251 < r on both curves
    return out


def interleaved(legs, reps=REPS):
    """legs: {name: fn}; one warm-up round, then `reps` rounds with the legs in turn -> {name: [seconds]}"""
    for fn in legs.values():
        fn()
    ts = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            t = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t)
    return ts


def fmt(ts, scale=1.0):
    v = [t * scale * 1e3 for t in ts]
    return f"{statistics.median(v):10.3f} ms [{min(v):.3f} .. {max(v):.3f}]"


def permute_loop(L, curve, states):
    """the caller's loop on the parent commit: one zl_poseidon_permute per state, in place"""
    base = states.ctypes.data
    u64p = C.POINTER(C.c_uint64)
    f = L.zl_poseidon_permute
    for i in range(states.shape[0]):
        f(curve, C.cast(base + 96 * i, u64p))


def hash2_by_loop(L, curve, xy):
    st = np.zeros((xy.shape[0], 3, 4), dtype=np.uint64)
    st[:, 0, 0] = 3
    st[:, 1:, :] = xy.reshape(-1, 2, 4)
    permute_loop(L, curve, st)
    return st[:, 0, :].copy()


def dev_tensor(a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def hash2_leg(be, curve, logs, threads, res):
    L, name = be.L, NAMES[curve]
    for lg in logs:
        n = 1 << lg
        xy = elems(2 * n, 100 + lg).reshape(n, 2, 4)
        d_xy, d_out = dev_tensor(xy), dev_tensor(np.zeros((n, 4), dtype=np.uint64))
        os.environ["ZL_TUNE_POSEIDON_DEV_MIN"] = "0"
        got = be.poseidon_hash2(curve, xy)
        be.poseidon_hash2_dev(curve, d_xy.data_ptr(), n, d_out.data_ptr())
        assert np.array_equal(d_out.cpu().numpy().view(np.uint64).reshape(n, 4), got)
        sample = np.arange(n) if n <= 4096 else np.random.default_rng(lg).choice(n, 256, replace=False)
        assert np.array_equal(hash2_by_loop(L, curve, xy[sample]), got[sample]), "device digests differ from the zl_poseidon_permute loop"
        if n <= (1 << 18):
            assert np.array_equal(zb.poseidon_hash2_host(curve, xy), got)
        m = min(n, 1 << 12)  # the loops: timed over m permutations, scaled to n
        st = np.zeros((m, 3, 4), dtype=np.uint64)
        st[:, 0, 0] = 3
        st[:, 1:, :] = xy[:m]
        parts = [st[i::threads].copy() for i in range(threads)] if m >= threads else [st.copy()]
        pool = ThreadPoolExecutor(max_workers=len(parts))

        def loop_t():
            list(pool.map(lambda p: permute_loop(L, curve, p), parts))

        legs = {"dev": lambda: be.poseidon_hash2_dev(curve, d_xy.data_ptr(), n, d_out.data_ptr()), "hostptr": lambda: be.poseidon_hash2(curve, xy),
                "loop1": lambda: permute_loop(L, curve, st.copy()), "loopT": loop_t}
        if n <= (1 << 18):
            legs["pool"] = lambda: zb.poseidon_hash2_host(curve, xy)
        ts = interleaved(legs)
        pool.shutdown()
        scale = n / m
        for k in ("loop1", "loopT"):
            ts[k] = [t * scale for t in ts[k]]
        best_old = min(min(ts["loop1"]), min(ts["loopT"]))
        row = {"curve": name, "log_n": lg}
        for k, v in ts.items():
            row[k + "_ms"] = statistics.median(v) * 1e3
            row[k + "_hashes_per_s"] = n / statistics.median(v)
        row["dev_fr_mul_per_s"] = 804 * n / statistics.median(ts["dev"])
        row["worst_speedup_hostptr_vs_best_loop"] = best_old / max(ts["hostptr"])
        row["worst_speedup_dev_vs_best_loop"] = best_old / max(ts["dev"])
        res["hash2"].append(row)
        say(f"hash2 {name} 2^{lg:<2d} dev {fmt(ts['dev'])} ({row['dev_hashes_per_s']:.3e} H/s, {row['dev_fr_mul_per_s']:.3e} Fr mul/s) | hostptr {fmt(ts['hostptr'])} "
            f"({row['hostptr_hashes_per_s']:.3e} H/s) | " + (f"pool {fmt(ts['pool'])} | " if "pool" in ts else "") +
            f"loop1 {fmt(ts['loop1'])} ({row['loop1_hashes_per_s']:.3e} H/s) | loopT({len(parts)}) {fmt(ts['loopT'])} | worst-case speedup over the faster loop: "
            f"hostptr {row['worst_speedup_hostptr_vs_best_loop']:.1f}x, dev {row['worst_speedup_dev_vs_best_loop']:.1f}x")


PRODUCTS = {3: 804, 4: 1288, 5: 1976, 6: 2616}  # 8 (3W + W^2) + partial (3 + W^2)


def permute_w_loop(L, curve, width, states):
    base = states.ctypes.data
    u64p = C.POINTER(C.c_uint64)
    f = L.zl_poseidon_permute_w
    for i in range(states.shape[0]):
        f(curve, width, C.cast(base + 32 * width * i, u64p))


def arity_leg(be, curve, logs, threads, res):
    L, name = be.L, NAMES[curve]
    for lg in logs:
        n = 1 << lg
        xy = elems(2 * n, 100 + lg).reshape(n, 2, 4)
        d_xy, d_h2 = dev_tensor(xy), dev_tensor(np.zeros((n, 4), dtype=np.uint64))
        for arity in (2, 3, 4, 5):
            width = arity + 1
            xs = elems(arity * n, 900 + 10 * lg + arity).reshape(n, arity, 4)
            d_in, d_out = dev_tensor(xs), dev_tensor(np.zeros((n, 4), dtype=np.uint64))
            os.environ["ZL_TUNE_POSEIDON_DEV_MIN"] = "0"
            got = be.poseidon_hash(curve, xs)
            be.poseidon_hash_dev(curve, arity, d_in.data_ptr(), n, d_out.data_ptr())
            assert np.array_equal(d_out.cpu().numpy().view(np.uint64).reshape(n, 4), got)
            sample = np.arange(n) if n <= 256 else np.random.default_rng(lg).choice(n, 256, replace=False)
            st = np.zeros((len(sample), width, 4), dtype=np.uint64)
            st[:, 0, 0] = (1 << arity) - 1
            st[:, 1:, :] = xs[sample]
            permute_w_loop(L, curve, width, st)
            assert np.array_equal(st[:, 0, :], got[sample]), "device digests differ from the zl_poseidon_permute_w loop"
            m = min(n, 1 << 12)
            lp = np.zeros((m, width, 4), dtype=np.uint64)
            lp[:, 0, 0] = (1 << arity) - 1
            lp[:, 1:, :] = xs[:m]
            parts = [lp[i::threads].copy() for i in range(threads)] if m >= threads else [lp.copy()]
            pool = ThreadPoolExecutor(max_workers=len(parts))

            def loop_t():
                list(pool.map(lambda p: permute_w_loop(L, curve, width, p), parts))

            legs = {"dev": lambda: be.poseidon_hash_dev(curve, arity, d_in.data_ptr(), n, d_out.data_ptr()), "hostptr": lambda: be.poseidon_hash(curve, xs),
                    "hash2_dev": lambda: be.poseidon_hash2_dev(curve, d_xy.data_ptr(), n, d_h2.data_ptr()), "hash2_hostptr": lambda: be.poseidon_hash2(curve, xy),
                    "loopT": loop_t}
            if n <= (1 << 10):
                legs["pool"] = lambda: zb.poseidon_hash_host(curve, xs)
            ts = interleaved(legs)
            pool.shutdown()
            ts["loopT"] = [t * (n / m) for t in ts["loopT"]]
            row = {"curve": name, "log_n": lg, "arity": arity, "width": width}
            for k, v in ts.items():
                row[k + "_ms"] = statistics.median(v) * 1e3
            row["dev_hashes_per_s"] = n / statistics.median(ts["dev"])
            row["hostptr_hashes_per_s"] = n / statistics.median(ts["hostptr"])
            row["dev_over_hash2_dev"] = statistics.median(ts["dev"]) / statistics.median(ts["hash2_dev"])
            row["worst_dev_over_hash2_dev"] = max(ts["dev"]) / min(ts["hash2_dev"])
            row["products_over_width3"] = PRODUCTS[width] / PRODUCTS[3]
            row["worst_speedup_hostptr_vs_loopT"] = min(ts["loopT"]) / max(ts["hostptr"])
            if "pool" in ts:
                row["device_wins_every_repetition_vs_pool"] = max(ts["hostptr"]) < min(ts["pool"])
            res["arity"].append(row)
            say(f"arity {name} arity {arity} (width {width}) 2^{lg:<2d} dev {fmt(ts['dev'])} ({row['dev_hashes_per_s']:.3e} H/s) | hostptr {fmt(ts['hostptr'])} "
                f"({row['hostptr_hashes_per_s']:.3e} H/s) | hash2 dev {fmt(ts['hash2_dev'])} | hash2 hostptr {fmt(ts['hash2_hostptr'])} | "
                + (f"pool {fmt(ts['pool'])} (device wins every repetition: {row['device_wins_every_repetition_vs_pool']}) | " if "pool" in ts else "")
                + f"loopT({len(parts)}) {fmt(ts['loopT'])} | dev / hash2 dev {row['dev_over_hash2_dev']:.2f} (worst pairing {row['worst_dev_over_hash2_dev']:.2f}; products "
                f"{row['products_over_width3']:.2f}) | worst-case speedup of hostptr over loopT {row['worst_speedup_hostptr_vs_loopT']:.1f}x")
            del d_in, d_out
        del d_xy, d_h2
        torch.cuda.empty_cache()


def devmin_leg(be, curve, res):
    name = NAMES[curve]
    wins = {}
    for lg in range(0, 13):
        n = 1 << lg
        xy = elems(2 * n, 300 + lg).reshape(n, 2, 4)

        def on_dev():
            os.environ["ZL_TUNE_POSEIDON_DEV_MIN"] = "0"
            return be.poseidon_hash2(curve, xy)

        def on_host():
            os.environ["ZL_TUNE_POSEIDON_DEV_MIN"] = str(1 << 30)
            return be.poseidon_hash2(curve, xy)

        assert np.array_equal(on_dev(), on_host())
        ts = interleaved({"dev": on_dev, "host": on_host})
        wins[lg] = max(ts["dev"]) < min(ts["host"])
        say(f"devmin {name} 2^{lg:<2d} device {fmt(ts['dev'])} | host path {fmt(ts['host'])} | device wins every repetition: {wins[lg]}")
    os.environ["ZL_TUNE_POSEIDON_DEV_MIN"] = "0"
    first = next((lg for lg in range(0, 13) if all(wins[x] for x in range(lg, 13))), None)
    res["devmin"].append({"curve": name, "smallest_log_count_device_always_wins": first})
    say(f"devmin {name}: smallest power of two from which the device wins every repetition: " + (f"2^{first} = {1 << first}" if first is not None else "none up to 2^12"))


def check_tree(be, curve, leaves, depth, d_nodes, root):
    L, n = be.L, leaves.shape[0]
    if n <= (1 << 16):
        nodes, hroot = zb.poseidon_merkle_build_host(curve, leaves, depth)
        assert np.array_equal(d_nodes.cpu().numpy().view(np.uint64).reshape(-1, 4), nodes) and np.array_equal(hroot, root)
        return
    idx = np.random.default_rng(n).choice(n, 32, replace=False).astype(np.uint64)
    paths = be.poseidon_merkle_paths(curve, d_nodes.data_ptr(), n, depth, idx)
    for i, p in zip(idx, paths):
        cur = leaves[int(i)]
        for k in range(depth):
            pair = np.stack([p[k], cur]) if (int(i) >> k) & 1 else np.stack([cur, p[k]])
            cur = hash2_by_loop(L, curve, pair.reshape(1, 2, 4))[0]
        assert np.array_equal(cur, root), "a gathered path does not fold to the device's root"


def merkle_leg(be, curve, logs, sweep_log, res):
    name = NAMES[curve]
    for lg in logs:
        n, depth = 1 << lg, max(1, lg)
        leaves = elems(n, 500 + lg)
        total = zb.poseidon_merkle_nodes(n, depth)
        d_leaves, d_nodes = dev_tensor(leaves), dev_tensor(np.zeros((total, 4), dtype=np.uint64))
        os.environ.pop("ZL_TUNE_POSEIDON_TAIL", None)
        root = be.poseidon_merkle_build_dev(curve, d_leaves.data_ptr(), n, depth, d_nodes.data_ptr())
        check_tree(be, curve, leaves, depth, d_nodes, root)

        def build(tail):
            def f():
                if tail is None:
                    os.environ.pop("ZL_TUNE_POSEIDON_TAIL", None)
                else:
                    os.environ["ZL_TUNE_POSEIDON_TAIL"] = str(tail)
                r = be.poseidon_merkle_build_dev(curve, d_leaves.data_ptr(), n, depth, d_nodes.data_ptr())
                assert np.array_equal(r, root)
            return f

        tails = [None] + ([0, 16, 64, 256, 1024] if lg == sweep_log else [0])
        ts = interleaved({("default" if t is None else str(t)): build(t) for t in tails})
        os.environ.pop("ZL_TUNE_POSEIDON_TAIL", None)
        row = {"curve": name, "log_n": lg, "hashes": total - n}
        for k, v in ts.items():
            row[f"tail_{k}_ms"] = statistics.median(v) * 1e3
        row["hashes_per_s_default"] = (total - n) / statistics.median(ts["default"])
        res["merkle"].append(row)
        say(f"merkle {name} 2^{lg:<2d} leaves ({total - n} hashes): " + " | ".join(f"T={k} {fmt(v)}" for k, v in ts.items()) +
            f" | {row['hashes_per_s_default']:.3e} H/s at the default")
        if lg == sweep_log:  # the levels above the threshold alone: a T-leaf tree with the tail kernel against a launch per level
            for T in (16, 64, 256, 1024):
                dT = max(1, T.bit_length() - 1)
                totT = zb.poseidon_merkle_nodes(T, dT)
                d_n2 = dev_tensor(np.zeros((totT, 4), dtype=np.uint64))

                def top(tail):
                    def f():
                        os.environ["ZL_TUNE_POSEIDON_TAIL"] = str(tail)
                        be.poseidon_merkle_build_dev(curve, d_leaves.data_ptr(), T, dT, d_n2.data_ptr())
                    return f

                tt = interleaved({"tail": top(T), "per_level": top(0)})
                os.environ.pop("ZL_TUNE_POSEIDON_TAIL", None)
                res["merkle_top"].append({"curve": name, "T": T, "tail_ms": statistics.median(tt["tail"]) * 1e3, "per_level_ms": statistics.median(tt["per_level"]) * 1e3})
                say(f"merkle-top {name} the {dT} levels above a {T}-node level: one tail launch {fmt(tt['tail'])} | a launch per level {fmt(tt['per_level'])} "
                    f"({statistics.median(tt['per_level']) / dT * 1e6:.1f} us per level)")
        del d_leaves, d_nodes
        torch.cuda.empty_cache()


def fold_leg(be, curve, log_leaves, counts_log, res):
    name = NAMES[curve]
    n, depth = 1 << log_leaves, log_leaves
    leaves = elems(n, 700)
    d_leaves, d_nodes = dev_tensor(leaves), dev_tensor(np.zeros((zb.poseidon_merkle_nodes(n, depth), 4), dtype=np.uint64))
    root = be.poseidon_merkle_build_dev(curve, d_leaves.data_ptr(), n, depth, d_nodes.data_ptr())
    os.environ["ZL_TUNE_POSEIDON_DEV_MIN"] = "0"
    for lg in counts_log:
        m = 1 << lg
        idx = np.random.default_rng(lg).integers(0, n, size=m, dtype=np.uint64)
        paths = be.poseidon_merkle_paths(curve, d_nodes.data_ptr(), n, depth, idx)
        lv = leaves[idx.astype(np.int64)]
        roots = be.poseidon_merkle_roots_from_paths(curve, lv, idx, paths, depth)
        assert (roots == root[None]).all()
        ts = interleaved({"fold": lambda: be.poseidon_merkle_roots_from_paths(curve, lv, idx, paths, depth),
                          "gather": lambda: be.poseidon_merkle_paths(curve, d_nodes.data_ptr(), n, depth, idx)})
        res["fold"].append({"curve": name, "depth": depth, "log_paths": lg, "fold_ms": statistics.median(ts["fold"]) * 1e3, "gather_ms": statistics.median(ts["gather"]) * 1e3,
                            "hashes_per_s": m * depth / statistics.median(ts["fold"])})
        say(f"fold {name} depth {depth} 2^{lg:<2d} paths: roots_from_paths {fmt(ts['fold'])} ({m * depth / statistics.median(ts['fold']):.3e} H/s) | "
            f"paths_dev gather {fmt(ts['gather'])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes only (a functional pass of every leg)")
    ap.add_argument("--arity", action="store_true", help="the arity leg alone (default output: profiles/poseidon_arity_bench.log)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "poseidon_arity_bench.log" if args.arity else "poseidon_bench.log")
    torch.cuda.init()
    be = Backend(0)
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    say(f"# {be.describe()}")
    say(f"# host threads granted: {threads}; repetitions: {REPS}; legs interleaved in one process")
    res = {"hash2": [], "devmin": [], "merkle": [], "merkle_top": [], "fold": [], "arity": []}
    for curve in (ZL_BLS12_381, ZL_BN254):
        if args.arity:
            arity_leg(be, curve, [6, 10] if args.quick else [6, 10, 14, 18, 22], threads, res)
            continue
        hash2_leg(be, curve, [6, 10] if args.quick else [6, 10, 14, 18, 22], threads, res)
        devmin_leg(be, curve, res)
        merkle_leg(be, curve, [10, 12] if args.quick else [10, 16, 20, 24], 12 if args.quick else 20, res)
        fold_leg(be, curve, 12 if args.quick else 20, [6, 10] if args.quick else [10, 16], res)
    say(json.dumps(res))
    be.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LOG) + "\n")


if __name__ == "__main__":
    main()
