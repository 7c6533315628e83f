"""Cost of proving hybrid encryptions (zl_hybrid_encrypt_assignments, zl_groth16_prove_hybrid_encryptions), both curves, (W; H, N) = (3; 0, 1).

  python tools/hybrid_prove_bench.py [--quick] [--curves bls12_381,bn254] [--out profiles/hybrid_prove_bench.log]

Every leg is checked before it is timed, the legs of a line are interleaved in one process, five repetitions after one warm-up round; a line gives the median,
[min .. max], and ratios on the WORST pairing of repetitions (slowest run of the new call against the fastest run of the other side).

  (a) trace    the assignments alone at 2^6 .. 2^14 rows, at full width and at bits = 64: (dev) k_ed_hybrid_ladders + k_pos_duplex_trace_in on device operands,
               rows left on the device, (pool) ctx == NULL: the host mirror over the host pool, timed over at most 2^8 rows and scaled (equal, independent rows).
               128, 256 and 512 rows are the sizes around ZL_TUNE_ED_DEV_MIN = 256.
  (b) proofs   prove_hybrid_encryptions at 64 and 1 024 proofs (bits = 32: a domain of 2^11, the device batch path; full width at 64 proofs: the resident
               loop) against what a caller must do without it, with this change's own circuit: one witness-only Circuit.hybrid_encrypt per proof on the host,
               then prove_batch over the rows.
Expected, from this repository's own logs (stated before the first run): the ladder launch costs about one k_ed_mul_trace launch -- 6.4 - 6.5 ms at full width up
to 2^10 rows (2^11 lanes: one wave per SIMD), 1.8 ms at 64 bits; the cipher launch at (3; 0, 1) about one k_pos_duplex_trace launch, 1.36 x 1.56 = 2.1 ms;
together about 8.6 ms at full width and 3.9 ms at 64 bits, flat while the ladder lanes fit one wave per SIMD."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402  (its HIP runtime initialises first, as in bench.py)

from ed_prove_bench import masked, subgroup_points  # noqa: E402
from edwards_bench import NAMES, a_point, dev_tensor, env, fmt, interleaved, scalars  # noqa: E402
from openzl_amd import ZL_BLS12_381, ZL_BN254, Backend, Circuit, Groth16Keys  # noqa: E402
from openzl_amd import backend as zb  # noqa: E402

HOST_CAP = 1 << 8
W, H, N = 3, 0, 1
LOG = []
SATURATED = [0]
EXPECT_MS = {64: 1.8 + 2.1}  # full width: 6.45 + 2.1


def say(line):
    print(line, flush=True)
    LOG.append(line)


def as_int(w):
    return sum(int(v) << (64 * i) for i, v in enumerate(w))


def operands(be, curve, g, n, bits, seed):
    """(esk, pks, headers, plaintexts) of n messages, each to its own recipient"""
    texts = scalars(curve, n * N * (W - 1), seed + 2).reshape(n, N, W - 1, 4)  # (< 2^250: below r)
    return masked(curve, n, bits, seed), subgroup_points(be, curve, g, n, seed + 1), np.zeros((n, H, 4), dtype=np.uint64), texts


def trace_leg(be, curve, g, bits, logs, wins):
    nv = zb.hybrid_encrypt_assignment_elems(curve, W, bits, H, N)
    full = bits == zb.ed_order_bits(curve)
    for lg in logs:
        n = 1 << lg
        esk, pks, hd, tx = operands(be, curve, g, n, bits, 10 + 3 * lg)
        hm = min(n, HOST_CAP)
        d_e, d_p, d_t = dev_tensor(esk), dev_tensor(pks), dev_tensor(tx)
        d_o = torch.zeros(n * nv * 4, dtype=torch.int64, device="cuda")
        run = lambda: be.hybrid_encrypt_assignments_dev(curve, W, bits, None, g, d_e.data_ptr(), d_p.data_ptr(), 1, 0, H, d_t.data_ptr(), N, n, d_o.data_ptr())
        run()
        m = min(n, 64)
        exp = zb.hybrid_encrypt_assignments_host(curve, None, g, esk[:m], pks[:m], hd[:m], tx[:m], bits)
        assert np.array_equal(d_o[:m * nv * 4].cpu().numpy().view(np.uint64).reshape(m, nv, 4), exp), "device and host mirror differ"
        legs = {"dev": run, "pool": lambda: zb.hybrid_encrypt_assignments_host(curve, None, g, esk[:hm], pks[:hm], hd[:hm], tx[:hm], bits)}
        ts = interleaved(legs)
        scale = n / hm
        worst = min(ts["pool"]) * scale / max(ts["dev"])
        med = statistics.median(ts["pool"]) * scale / statistics.median(ts["dev"])
        wins.setdefault((bits, lg), []).append(worst > 1.0)
        got = statistics.median(ts["dev"]) * 1e3
        exp_ms = 6.45 + 2.1 if full else EXPECT_MS[bits]
        flat = 2 * n <= SATURATED[0]
        say(f"(a) {NAMES[curve]} bits={bits} 2^{lg} rows ({n * nv * 32 / 2**20:.1f} MiB): dev {fmt(ts['dev'])}  pool {fmt(ts['pool'], scale)}  "
            f"x {med:.2f} median, x {worst:.2f} worst pairing{'  ** LOSS **' if worst < 1.0 else ''}")
        say(f"      expected {exp_ms:.2f} ms (one k_ed_mul_trace launch + one k_pos_duplex_trace launch{'' if flat else '; beyond one wave per SIMD, not flat'}): "
            f"measured {got:.3f} ms, {100.0 * (got - exp_ms) / exp_ms:+.1f} %")
        del d_o


def proof_leg(be, curve, g, bits, counts):
    esk0, pk0, hd0, tx0 = operands(be, curve, g, 1, bits, 5)
    pt = lambda w: (as_int(w[0]), as_int(w[1]))
    blocks = lambda t: [[as_int(v) for v in blk] for blk in t]
    gi = pt(g)
    full = Circuit.hybrid_encrypt(curve, None, gi, as_int(esk0[0]), pt(pk0[0]), [], blocks(tx0[0]), bits)
    keys = Groth16Keys(be, full, seed=77)
    dom = 1 << max(1, (full.shape[0] + full.shape[1] - 1).bit_length())
    try:
        for n in counts:
            esk, pks, hd, tx = operands(be, curve, g, n, bits, 100 + n)
            r, s = scalars(curve, n, 300 + n), scalars(curve, n, 400 + n)
            env(ZL_TUNE_ED_DEV_MIN=None)

            def today():
                rows = []
                for j in range(n):
                    c = Circuit.hybrid_encrypt(curve, None, gi, as_int(esk[j]), pt(pks[j]), [], blocks(tx[j]), bits, witness_only=True)
                    rows.append(c.arrays()["assignment"])
                    c.close()
                return keys.prove_batch(np.stack(rows), r, s)

            def fused():
                return keys.prove_hybrid_encryptions(None, g, esk, pks, hd, tx, r, s, bits=bits)[0]

            a, b = fused(), today()
            assert all(np.array_equal(np.asarray(x), np.asarray(y)) for p, q in zip(a, b) for x, y in zip(p, q)), "the two routes give different proofs"
            ts = interleaved({"fused": fused, "today": today}, reps=3 if n >= 1024 else 5)
            worst, med = min(ts["today"]) / max(ts["fused"]), statistics.median(ts["today"]) / statistics.median(ts["fused"])
            say(f"(b) {NAMES[curve]} bits={bits} (domain 2^{dom.bit_length() - 1}) {n} proofs: prove_hybrid_encryptions {fmt(ts['fused'])}  circuits + prove_batch {fmt(ts['today'])}  "
                f"x {med:.2f} median, x {worst:.2f} worst pairing{'  ** LOSS **' if worst < 1.0 else ''}")
    finally:
        keys.close()
        full.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="2^6 .. 2^10 and 2^14 rows; 64 proofs")
    ap.add_argument("--curves", default="bls12_381,bn254")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hybrid_prove_bench.log"))
    args = ap.parse_args()
    be = Backend(0)
    say(be.describe())
    props = torch.cuda.get_device_properties(0)
    SATURATED[0] = props.multi_processor_count * 4 * 64
    say(f"lanes at one wave per SIMD: {SATURATED[0]} (two lanes a row); host pool legs on {os.cpu_count()} logical CPUs (OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')})")
    logs = (6, 7, 8, 9, 10, 14) if args.quick else tuple(range(6, 15))
    wins = {}
    try:
        for curve in (ZL_BLS12_381, ZL_BN254):
            if NAMES[curve] not in args.curves.split(","):
                continue
            g = a_point(curve)
            full = zb.ed_order_bits(curve)
            for bits in (full, 64):
                trace_leg(be, curve, g, bits, logs, wins)
            proof_leg(be, curve, g, 32, (64,) if args.quick else (64, 1024))
            proof_leg(be, curve, g, full, (64,))
        for bits in sorted({b for b, _ in wins}):
            won = None
            for lg in sorted((lg for b, lg in wins if b == bits), reverse=True):
                if not all(v for (b, l2), vs in wins.items() if b == bits and l2 == lg for v in vs):
                    break
                won = lg
            say(f"trace at bits={bits}: " + (f"the device won every repetition from 2^{won} rows" if won is not None else "the device lost at the largest size measured"))
    finally:
        be.close()
    with open(args.out, "w") as f:  # only a complete run replaces the log
        f.write("\n".join(LOG) + "\n")


if __name__ == "__main__":
    main()
