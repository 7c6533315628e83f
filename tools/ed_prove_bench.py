"""Cost of proving embedded-curve scalar multiplications (zl_ed_scalar_mul_assignments, zl_groth16_prove_ed_scalar_muls), both curves.

  python tools/ed_prove_bench.py [--quick] [--out profiles/ed_prove_bench.log]

Every leg is checked before it is timed, the legs of a line are interleaved in one process, five repetitions after one warm-up round; a line gives the median,
[min .. max], and ratios on the WORST pairing of repetitions (slowest run of the new call against the fastest run of the other side).

  (a) trace    the assignments alone at 2^6 .. 2^14 rows, at full width and at bits = 64: (dev) k_ed_mul_trace on device operands, rows left on the device,
               (pool) ctx == NULL: the same text over the host pool, timed over at most 2^8 rows and scaled (equal, independent rows).
  (b) proofs   prove_scalar_muls at 64 and 1 024 proofs (bits = 64: the device batch path; full width at 64 proofs: the resident loop) against what a caller
               had to do without it: one witness-only Circuit.ed_scalar_mul per proof on the host, then prove_batch over the rows.
Derived: the expected time of the (dev) leg.  A step costs 19 + 12 + 18 dependent products (ladder, Montgomery's trick, records), the inversion 380: 49 (bits -
1) + 380, 12 679 at bits = 252, against the 9 000 estimated before the kernel existed; at the 804 products / 0.42 ms of a width-3 permutation that is 6.6 ms (5 ms for the
estimate) up to one wave per SIMD, and the deviation of the measurement from both."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402  (its HIP runtime initialises first, as in bench.py)

from edwards_bench import NAMES, a_point, dev_tensor, env, fmt, interleaved, scalars  # noqa: E402
from openzl_amd import ZL_BLS12_381, ZL_BN254, Backend, Circuit, Groth16Keys  # noqa: E402
from openzl_amd import backend as zb  # noqa: E402

HOST_CAP = 1 << 8
LOG = []
SATURATED = [0]
MS_PER_PRODUCT = 0.42 / 804


def say(line):
    print(line, flush=True)
    LOG.append(line)


def products(bits):
    return 49 * (bits - 1) + 380


def masked(curve, n, bits, seed):
    """n scalars below 2^bits and below l"""
    ks = scalars(curve, n, seed)  # < 2^250
    for w in range(4):
        lo = 64 * w
        ks[:, w] &= np.uint64(0 if bits <= lo else (1 << min(64, bits - lo)) - 1)
    return ks


def subgroup_points(be, curve, g, n, seed):
    env(ZL_TUNE_ED_DEV_MIN="0", ZL_TUNE_ED_FIXED_MIN="0")
    pts, st = be.ed_scalar_mul(curve, g, scalars(curve, n, seed))
    assert not st.any()
    return pts


def trace_leg(be, curve, g, bits, logs, wins):
    nv = zb.ed_scalar_mul_assignment_elems(curve, bits)
    for lg in logs:
        n = 1 << lg
        pts, ks = subgroup_points(be, curve, g, n, 10 + lg), masked(curve, n, bits, 40 + lg)
        hm = min(n, HOST_CAP)
        d_p, d_k = dev_tensor(pts), dev_tensor(ks)
        d_o = torch.zeros(n * nv * 4, dtype=torch.int64, device="cuda")
        be.ed_scalar_mul_assignments_dev(curve, bits, d_p.data_ptr(), 1, d_k.data_ptr(), n, d_o.data_ptr())
        m = min(n, 64)
        exp = zb.ed_scalar_mul_assignments_host(curve, pts[:m], ks[:m], bits)
        assert np.array_equal(d_o[:m * nv * 4].cpu().numpy().view(np.uint64).reshape(m, nv, 4), exp), "device and host mirror differ"
        legs = {"dev": lambda: be.ed_scalar_mul_assignments_dev(curve, bits, d_p.data_ptr(), 1, d_k.data_ptr(), n, d_o.data_ptr()),
                "pool": lambda: zb.ed_scalar_mul_assignments_host(curve, pts[:hm], ks[:hm], bits)}
        ts = interleaved(legs)
        scale = n / hm
        worst = min(ts["pool"]) * scale / max(ts["dev"])
        med = statistics.median(ts["pool"]) * scale / statistics.median(ts["dev"])
        wins.setdefault((bits, lg), []).append(worst > 1.0)
        fill = max(1.0, n / SATURATED[0])
        got = statistics.median(ts["dev"]) * 1e3
        own, early = products(bits) * MS_PER_PRODUCT * fill, 9000 * (bits - 1) / 251 * MS_PER_PRODUCT * fill
        say(f"(a) {NAMES[curve]} bits={bits} 2^{lg} rows ({n * nv * 32 / 2**20:.1f} MiB): dev {fmt(ts['dev'])}  pool {fmt(ts['pool'], scale)}  "
            f"x {med:.2f} median, x {worst:.2f} worst pairing{'  ** LOSS **' if worst < 1.0 else ''}")
        say(f"      expected {own:.3f} ms ({products(bits)} products) / {early:.3f} ms (the 9 000-product estimate, scaled to the width): measured {got:.3f} ms, "
            f"{100.0 * (got - own) / own:+.1f} % / {100.0 * (got - early) / early:+.1f} %")
        del d_o


def proof_leg(be, curve, g, bits, counts):
    pt0 = subgroup_points(be, curve, g, 1, 5)[0]
    k0 = masked(curve, 1, bits, 6)[0]
    as_int = lambda w: sum(int(v) << (64 * i) for i, v in enumerate(w))
    full = Circuit.ed_scalar_mul(curve, (as_int(pt0[0]), as_int(pt0[1])), as_int(k0), bits)
    keys = Groth16Keys(be, full, seed=77)
    try:
        for n in counts:
            pts, ks = subgroup_points(be, curve, g, n, 100 + n), masked(curve, n, bits, 200 + n)
            r, s = scalars(curve, n, 300 + n), scalars(curve, n, 400 + n)
            env(ZL_TUNE_ED_DEV_MIN=None)

            def today():
                rows = []
                for j in range(n):
                    c = Circuit.ed_scalar_mul(curve, (as_int(pts[j, 0]), as_int(pts[j, 1])), as_int(ks[j]), bits, witness_only=True)
                    rows.append(c.arrays()["assignment"])
                    c.close()
                return keys.prove_batch(np.stack(rows), r, s)

            def fused():
                return keys.prove_scalar_muls(pts, ks, r, s, bits=bits)[0]

            a, b = fused(), today()
            assert all(np.array_equal(np.asarray(x), np.asarray(y)) for p, q in zip(a, b) for x, y in zip(p, q)), "the two routes give different proofs"
            ts = interleaved({"fused": fused, "today": today}, reps=3 if n >= 1024 else 5)
            worst, med = min(ts["today"]) / max(ts["fused"]), statistics.median(ts["today"]) / statistics.median(ts["fused"])
            say(f"(b) {NAMES[curve]} bits={bits} {n} proofs: prove_scalar_muls {fmt(ts['fused'])}  circuits + prove_batch {fmt(ts['today'])}  "
                f"x {med:.2f} median, x {worst:.2f} worst pairing{'  ** LOSS **' if worst < 1.0 else ''}")
    finally:
        keys.close()
        full.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="2^6, 2^10 and 2^14 rows; 64 proofs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ed_prove_bench.log"))
    args = ap.parse_args()
    be = Backend(0)
    say(be.describe())
    props = torch.cuda.get_device_properties(0)
    SATURATED[0] = props.multi_processor_count * 4 * 64
    say(f"lanes at one wave per SIMD: {SATURATED[0]}; host pool legs on {os.cpu_count()} logical CPUs (OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')})")
    logs = (6, 10, 14) if args.quick else tuple(range(6, 15))
    wins = {}
    try:
        for curve in (ZL_BLS12_381, ZL_BN254):
            g = a_point(curve)
            full = zb.ed_order_bits(curve)
            for bits in (full, 64):
                trace_leg(be, curve, g, bits, logs, wins)
            proof_leg(be, curve, g, 64, (64,) if args.quick else (64, 1024))
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
