"""The fused encryption prover against what a caller writes without it, both curves.

  python tools/poseidon_encrypt_prove_bench.py [--quick] [--counts 64,1024,16384] [--resident-max N] [--no-traces] [--out profiles/poseidon_encrypt_prove_bench.log]

  fused    Groth16Keys.prove_encryptions: keys, headers and plaintexts in; proofs, tags and ciphertexts out -- the cipher runs once, on the device, under a recorder
  loop     one witness-only Circuit.poseidon_encrypt per proof, its assignment copied out, then Groth16Keys.prove_batch over the stacked assignments:
           synthesis on the host, the assignments over the bus.  Tag and ciphertext are read out of the assignments
  cipher+loop   Backend.poseidon_duplex_encrypt for the tags and ciphertexts, then the loop: what a caller that encrypts on the device and proves each
           ciphertext well formed does today -- the cipher runs twice
Shapes (W, K, H, N): (3, 2, 0, 1) and (6, 2, 0, 1) -- 948 and 930 constraints, domain 2^10 -- and the eight-block (4, 2, 0, 8), domain 2^12, which loops the
resident prover in every leg.  Dispatch is the library's own (no ZL_TUNE_* set).  Before anything is timed the fused proofs, tags and ciphertexts of every shape
are checked against the loop's and the cipher's, byte for byte.  The legs are interleaved in one process, five repetitions after one warm-up round; a line
gives the median, [min .. max], proofs/s at the median and the speedup on the WORST pairing (slowest fused call against the fastest run of the other leg).

  trace    k_pos_duplex_trace alone against k_pos_duplex alone, device operands, the same shapes, 2^10 .. 2^16 rows, interleaved: what recording and
           writing the rows costs over the cipher (profiles/poseidon_duplex_bench.log has the cipher's times from its own run)."""
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

from openzl_amd import ZL_BLS12_381, ZL_BN254, Backend, Circuit, Groth16Keys, poseidon_duplex_permutations, poseidon_encrypt_assignment_elems  # noqa: E402

NAMES = {ZL_BLS12_381: "bls12_381", ZL_BN254: "bn254"}
SHAPES = [(3, 2, 0, 1), (6, 2, 0, 1), (4, 2, 0, 8)]
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


def prove(be, curve, shape, counts, reps, res, resident_max):
    name = NAMES[curve]
    width, kl, hl, n = shape
    rate = width - 1
    nv = poseidon_encrypt_assignment_elems(width, kl, hl, n)
    log_n = (nv - kl).bit_length()  # the domain holds n_constraints + n_instance = nv - K + 1 rows
    if resident_max and log_n > 11:
        skipped = [c for c in counts if c > resident_max]
        counts = [c for c in counts if c <= resident_max]
        if skipped:
            say(f"{name:9s} W={width} (K, H, N)=({kl}, {hl}, {n}): counts {skipped} skipped (--resident-max {resident_max})")
        if not counts:
            return
    top = max(counts)
    st = elems(width, 70 + width)
    k, h, t = elems(top * kl, 71).reshape(top, kl, 4), elems(top * hl, 72).reshape(top, hl, 4), elems(top * n * rate, 73).reshape(top, n, rate, 4)
    sti = ints(st)
    ki, hi, ti = [ints(row) for row in k], [ints(row) for row in h], [[ints(b) for b in item] for item in t]
    r, s = elems(top, 74), elems(top, 75)
    full = Circuit.poseidon_encrypt(curve, sti, ki[0], hi[0], ti[0])
    keys = Groth16Keys(be, full, seed=47)

    def loop(c):
        rows = []
        for j in range(c):
            w = Circuit.poseidon_encrypt(curve, sti, ki[j], hi[j], ti[j], witness_only=True)
            rows.append(w.arrays()["assignment"])
            w.close()
        z = np.stack(rows)
        return keys.prove_batch(z, r[:c], s[:c]), z[:, 1], z[:, 2:2 + n * rate]

    def cipher_loop(c):
        cts, tags = be.poseidon_duplex_encrypt(curve, st, k[:c], h[:c], t[:c])
        return loop(c)[0], tags, cts

    def fused(c):
        return keys.prove_encryptions(st, k[:c], h[:c], t[:c], r[:c], s[:c])

    c0 = min(70, top)
    got, tags, cts = fused(c0)
    exp, etags, ects = loop(c0)
    cct, ctg = be.poseidon_duplex_encrypt(curve, st, k[:c0], h[:c0], t[:c0])
    assert all(same(a, b) for a, b in zip(got, exp)), "fused proofs differ from the loop's"
    assert np.array_equal(tags, etags) and np.array_equal(tags, ctg) and np.array_equal(cts, cct) and np.array_equal(cts.reshape(c0, -1, 4), ects)
    for c in counts:
        ts = interleaved({"fused": lambda: fused(c), "loop": lambda: loop(c), "cipher+loop": lambda: cipher_loop(c)}, reps)
        row = {"curve": name, "circuit": "encrypt", "width": width, "key_len": kl, "header_len": hl, "blocks": n, "log_n": log_n, "count": c}
        say(f"{name:9s} W={width} (K, H, N)=({kl}, {hl}, {n}) domain 2^{log_n}  {c:6d} proofs")
        for leg, v in ts.items():
            med = statistics.median(v)
            row[leg + "_ms"] = med * 1e3
            line = f"    {leg:12s} {fmt(v)}  {c / med:12.0f} proofs/s"
            if leg != "fused":
                row["fused_worst_speedup_vs_" + leg] = min(v) / max(ts["fused"])
                line += f"   fused on the worst pairing {min(v) / max(ts['fused']):7.2f}x"
            say(line)
        res.append(row)
    keys.close()
    full.close()


def traces(be, curve, logs, reps, res):
    """the trace kernel and the cipher kernel alone: device operands in, dense rows resp. ciphertexts and tags out"""
    name = NAMES[curve]
    for width, kl, hl, n in SHAPES:
        rate = width - 1
        perms = poseidon_duplex_permutations(width, kl, hl, n)
        nv = poseidon_encrypt_assignment_elems(width, kl, hl, n)
        for log in logs:
            rows = 1 << log
            if rows * nv * 32 > (6 << 30):
                say(f"{name:9s} trace W={width} (K, H, N)=({kl}, {hl}, {n}) 2^{log}: skipped, {rows * nv * 32 >> 20} MiB of rows")
                continue
            d_k, d_h, d_t = dev(elems(rows * kl, 81 + log)), dev(elems(max(1, rows * hl), 82 + log)), dev(elems(rows * n * rate, 83 + log))
            d_out = torch.empty((rows, nv, 4), dtype=torch.int64, device="cuda")
            d_ct = torch.empty((rows, n * rate, 4), dtype=torch.int64, device="cuda")
            d_tag = torch.empty((rows, 4), dtype=torch.int64, device="cuda")
            legs = {"trace": lambda: be.poseidon_encrypt_assignments_dev(curve, width, None, d_k.data_ptr(), kl, d_h.data_ptr(), hl, d_t.data_ptr(), n, rows, d_out.data_ptr()),
                    "cipher": lambda: be.poseidon_duplex_encrypt_dev(curve, width, None, d_k.data_ptr(), kl, d_h.data_ptr(), hl, d_t.data_ptr(), n, rows, d_ct.data_ptr(),
                                                                       d_tag.data_ptr())}
            ts = interleaved(legs, reps)
            tm, cm = statistics.median(ts["trace"]) * 1e3, statistics.median(ts["cipher"]) * 1e3
            say(f"{name:9s} trace W={width} (K, H, N)=({kl}, {hl}, {n}) {perms} permutations 2^{log:<2d} rows: trace {tm:8.3f} (max {max(ts['trace']) * 1e3:.3f})  "
                f"k_pos_duplex {cm:8.3f} (max {max(ts['cipher']) * 1e3:.3f}) ms   +{(tm - cm) / perms:.3f} ms per permutation, {tm / cm:.2f}x")
            res.append({"curve": name, "circuit": "trace", "width": width, "key_len": kl, "header_len": hl, "blocks": n, "rows": rows, "trace_ms": tm,
                        "trace_max_ms": max(ts["trace"]) * 1e3, "cipher_ms": cm, "cipher_max_ms": max(ts["cipher"]) * 1e3})
            del d_out, d_ct, d_tag


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="counts 64 and 1024, traces at 2^10 and 2^14: a few minutes")
    ap.add_argument("--counts", default=None, help="comma-separated proof counts (default 64,1024,16384)")
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--resident-max", type=int, default=0, help="largest count run for a shape whose domain is above 2^11 (every leg loops the resident prover); 0 = all")
    ap.add_argument("--no-traces", action="store_true", help="leave out the trace-kernel legs")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    counts = [int(c) for c in args.counts.split(",")] if args.counts else ([64, 1024] if args.quick else [64, 1024, 16384])
    torch.cuda.init()
    for k in ("ZL_TUNE_G16_BATCH_LOG_N", "ZL_TUNE_G16_BATCH_MIN", "ZL_TUNE_G16_BATCH_CHUNK", "ZL_TUNE_POSEIDON_DEV_MIN", "ZL_TUNE_POSEIDON_CHUNK"):
        os.environ.pop(k, None)
    be = Backend(0)
    res = []
    say(f"# poseidon_encrypt_prove_bench: {torch.cuda.get_device_name(0)}, {args.reps} repetitions after one warm-up round, legs interleaved, counts {counts}")
    for curve in (ZL_BLS12_381, ZL_BN254):
        for shape in SHAPES:
            prove(be, curve, shape, counts, args.reps, res, args.resident_max)
            if args.out:  # (kept current: a long run that is cut short leaves what it measured)
                with open(args.out, "w") as f:
                    f.write("\n".join(LOG) + "\n")
        if not args.no_traces:
            traces(be, curve, (10, 14) if args.quick else (10, 12, 14, 16), args.reps, res)
    say("JSON " + json.dumps(res))
    be.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LOG) + "\n")


if __name__ == "__main__":
    main()
