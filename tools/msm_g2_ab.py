#!/usr/bin/env python3
"""One side of an interleaved A/B of G2 MSM sizes (tools/ab/bn254_g2_gls_ab.sh; log: profiles/bn254_g2_gls_ab.log).

  python tools/msm_g2_ab.py TAG [log_n ...]    one process: per size, single-call and pipelined (batch of 8) wall times of a BN254 G2 MSM over device-resident
                                               scalars.  ZL_BACKEND_LIB=<library> selects the build under test (the parent commit's for the "parent" side).
  python tools/msm_g2_ab.py --digest LOG       per size and mode: the best time of every run of each tag, their ratio, and the run-to-run spread of each tag
"""
import os
import re
import sys
import time
from collections import defaultdict


def digest(path):
    runs = defaultdict(lambda: defaultdict(list))  # (what, size) -> tag -> [ms per run]
    for line in open(path):
        m = re.match(r"\[(\w+)\] (msm 2\^\d+ (?:single|batch8)|prove k=\d+)\s*(?:c=\s*\d+)?\s*:? *min\s+([0-9.]+)", line)
        if m:
            runs[m.group(2)][m.group(1)].append(float(m.group(3)))
    tags = sorted({t for v in runs.values() for t in v})
    print(f"{'':24s}" + "".join(f"{t + ' (best of runs)':>26s}{'spread':>9s}" for t in tags) + f"{tags[-1] + ' / ' + tags[0]:>16s}")
    for what, by_tag in runs.items():
        row = f"{what:24s}"
        best = {}
        for t in tags:
            v = by_tag.get(t, [])
            if not v:
                row += f"{'-':>26s}{'':>9s}"
                continue
            best[t] = min(v)
            row += f"{min(v):23.3f} ms{(max(v) - min(v)) / min(v) * 100:7.1f} %"
        if len(best) == len(tags):
            row += f"{best[tags[-1]] / best[tags[0]]:16.3f}"
        print(row)


def main():
    if sys.argv[1] == "--digest":
        return digest(sys.argv[2])
    tag = sys.argv[1]
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    from bench import random_scalars_lt_r
    from openzl_amd import Backend, ZL_BN254, ZL_G2

    R_BN = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
    sizes = [int(a) for a in sys.argv[2:]] or list(range(8, 21))
    be = Backend(0)
    be.enable_timing(True)
    nmax = 1 << max(sizes)
    s = torch.from_numpy(random_scalars_lt_r(nmax, 2, R_BN, 254).view(np.int64)).to(torch.device("cuda", 0))
    k = random_scalars_lt_r(nmax, 1, R_BN, 254)
    for ln in sizes:
        n = 1 << ln
        h = be.bases_generate(ZL_BN254, k[:n], group=ZL_G2)  # one handle per size: the images kept with the handle cover exactly this range
        for _ in range(3):
            be.msm_dev(h, s.data_ptr(), n)
        reps = 40 if ln <= 14 else (12 if ln <= 18 else 6)
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            be.msm_dev(h, s.data_ptr(), n)
            ts.append((time.perf_counter() - t0) * 1e3)
        c = be.last_timing().window_bits
        ts.sort()
        print(f"[{tag}] msm 2^{ln} single c={c:2d}: min {ts[0]:9.4f} ms  median {ts[len(ts) // 2]:9.4f} ms", flush=True)
        be.msm_batch_partial_dev(h, [s.data_ptr()] * 8, n)
        tb = []
        for _ in range(max(3, reps // 4)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            be.msm_batch_partial_dev(h, [s.data_ptr()] * 8, n)
            tb.append((time.perf_counter() - t0) * 1e3 / 8)
        tb.sort()
        print(f"[{tag}] msm 2^{ln} batch8 c={be.last_timing().window_bits:2d}: min {tb[0]:9.4f} ms  median {tb[len(tb) // 2]:9.4f} ms  (per MSM)", flush=True)
        be.bases_free(h)


if __name__ == "__main__":
    main()
