"""Throughput of the embedded-curve scalar multiplication and the hybrid decryption scan (zl_ed_scalar_mul_batch, zl_hybrid_decrypt_batch), both curves.

  python tools/edwards_bench.py [--quick] [--out profiles/edwards_bench.log]

Every leg is checked before it is timed, the legs of a line are interleaved in one process, five repetitions after one warm-up round; a line gives the median,
[min .. max], and ratios on the WORST pairing of repetitions (slowest run of the new call against the fastest run of the other side).

  (a) variable base   per-item points and scalars at 2^6 .. 2^18 items: (dev) device operands, (hostptr) host operands through the device, copies included,
                      (pool) ctx == NULL: the host mirror over the host pool, timed over at most 2^10 items and scaled (equal, independent items).
  (b) shared base     one point for all items: (fixed) k_ed_mul_fixed, table build and upload included, (var) k_ed_mul on the same operands
                      (ZL_TUNE_ED_FIXED_MIN out of reach), (pool) as above.  Host operands.
  (c) scan            hybrid_decrypt with ONE secret key at (W, H, N) = (3, 0, 1), host operands, against today's route: the multiplications on the host pool
                      (timed over at most 2^10 items and scaled) plus poseidon_duplex_decrypt with the shared secrets uploaded as keys.
  bounds              host-pointer calls of 8 .. 256 items, device against pool (ZL_TUNE_ED_DEV_MIN), and the fixed-base kernel against k_ed_mul at every size
                      of (b) (ZL_TUNE_ED_FIXED_MIN): the bound is the smallest power of two from which the new path won EVERY repetition on both curves.
Derived: the expected time of the (dev) leg -- about 3 100 dependent products at the 804 products / 0.42 ms of a width-3 permutation: 1.6 ms (0.45 ms for the
fixed-base form's 800), times lanes / (CUs x 4 x 64) once every SIMD holds more than one wave -- and the deviation from it."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (its HIP runtime initialises first, as in bench.py)

from openzl_amd import ZL_BLS12_381, ZL_BN254, Backend  # noqa: E402
from openzl_amd import backend as zb  # noqa: E402

NAMES = {ZL_BLS12_381: "bls12_381", ZL_BN254: "bn254"}
MODULUS = {ZL_BLS12_381: 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001,
           ZL_BN254: 21888242871839275222246405745257275088548364400416034343698204186575808495617}
EXPECT_MS = {"var": 1.6, "fixed": 0.45}
REPS = 5
HOST_CAP = 1 << 10
HUGE = str(1 << 30)
LOG = []
SATURATED = [0]


def say(line):
    print(line, flush=True)
    LOG.append(line)


def words(vals):
    return np.array([[(v >> (64 * i)) & (2 ** 64 - 1) for i in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def a_point(curve):
    """one point of the prime-order subgroup: the first y = 2, 3, ... with an x on the curve, times the cofactor (through the library)"""
    q = MODULUS[curve]
    prm = zb.ed_params(curve)
    a, d = prm["a"], prm["d"]
    y = 2
    while True:
        x2 = (1 - y * y) * pow(a - d * y * y, -1, q) % q
        if pow(x2, (q - 1) // 2, q) == 1:
            break
        y += 1
    # Tonelli-Shanks
    s, t = 0, q - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    z = 2
    while pow(z, (q - 1) // 2, q) == 1:
        z += 1
    m, c, u, r = s, pow(z, t, q), pow(x2, t, q), pow(x2, (t + 1) // 2, q)
    while u != 1:
        i, w = 0, u
        while w != 1:
            w, i = w * w % q, i + 1
        b = pow(c, 1 << (m - i - 1), q)
        m, c, u, r = i, b * b % q, u * b * b % q, r * b % q
    p = words([r, y]).reshape(2, 4)
    out, st = zb.ed_scalar_mul_host(curve, p, words([prm["cofactor"]])[0], check_subgroup=False)
    assert not st.any()
    return out[0]


def scalars(curve, n, seed):
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 2 ** 63, size=(n, 4), dtype=np.uint64)
    out[:, 3] &= np.uint64((1 << 58) - 1)  # < 2^250 < l on both curves
    return out


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


def fmt(ts, scale=1.0):
    v = [t * scale * 1e3 for t in ts]
    return f"{statistics.median(v):10.3f} ms [{min(v):.3f} .. {max(v):.3f}]"


def ratio(ts, new, old, scale):
    worst = min(ts[old]) * scale.get(old, 1.0) / (max(ts[new]) * scale.get(new, 1.0))
    med = statistics.median(ts[old]) * scale.get(old, 1.0) / (statistics.median(ts[new]) * scale.get(new, 1.0))
    return med, worst


def dev_tensor(a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    return t


def env(**kv):
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def variable_leg(be, curve, g, logs):
    for lg in logs:
        n = 1 << lg
        env(ZL_TUNE_ED_DEV_MIN="0", ZL_TUNE_ED_FIXED_MIN="0")
        pts, _ = be.ed_scalar_mul(curve, g, scalars(curve, n, 10 + lg))  # n points of the subgroup
        ks = scalars(curve, n, 40 + lg)
        out, st = be.ed_scalar_mul(curve, pts, ks)
        m = min(n, 256)
        assert not st.any() and np.array_equal(out[:m], zb.ed_scalar_mul_host(curve, pts[:m], ks[:m])[0]), "device and host mirror differ"
        d_p, d_k, d_o, d_s = dev_tensor(pts), dev_tensor(ks), dev_tensor(np.zeros_like(pts)), dev_tensor(np.zeros(n, dtype=np.uint8))
        hm = min(n, HOST_CAP)
        legs = {"dev": lambda: be.ed_scalar_mul_dev(curve, d_p.data_ptr(), 1, d_k.data_ptr(), 1, n, d_o.data_ptr(), d_s.data_ptr()),
                "hostptr": lambda: be.ed_scalar_mul(curve, pts, ks),
                "pool": lambda: zb.ed_scalar_mul_host(curve, pts[:hm], ks[:hm])}
        ts = interleaved(legs)
        scale = {"pool": n / hm}
        say(f"(a) {NAMES[curve]} variable base 2^{lg} items")
        for name in legs:
            say(f"    {name:8s} {fmt(ts[name], scale.get(name, 1.0))}")
        for new in ("dev", "hostptr"):
            med, worst = ratio(ts, new, "pool", scale)
            say(f"    {new} against (pool): x {med:.2f} median, x {worst:.2f} worst pairing{'  ** LOSS **' if worst < 1.0 else ''}")
        fill = max(1.0, n / SATURATED[0])
        expect, got = EXPECT_MS["var"] * fill, statistics.median(ts["dev"]) * 1e3
        say(f"    expected 1.6 ms x {fill:g} (lanes over one wave per SIMD) = {expect:.3f} ms, dev measured {got:.3f} ms: {100.0 * (got - expect) / expect:+.1f} %")


def shared_leg(be, curve, g, logs, wins):
    for lg in logs:
        n = 1 << lg
        ks = scalars(curve, n, 70 + lg)
        env(ZL_TUNE_ED_DEV_MIN="0", ZL_TUNE_ED_FIXED_MIN="0")
        out, st = be.ed_scalar_mul(curve, g, ks)
        env(ZL_TUNE_ED_FIXED_MIN=HUGE)
        out_v, _ = be.ed_scalar_mul(curve, g, ks)
        m = min(n, 256)
        assert not st.any() and np.array_equal(out, out_v) and np.array_equal(out[:m], zb.ed_scalar_mul_host(curve, g, ks[:m])[0]), "the shared-base paths differ"
        hm = min(n, HOST_CAP)

        def fixed():
            env(ZL_TUNE_ED_FIXED_MIN="0")
            be.ed_scalar_mul(curve, g, ks)

        def var():
            env(ZL_TUNE_ED_FIXED_MIN=HUGE)
            be.ed_scalar_mul(curve, g, ks)

        legs = {"fixed": fixed, "var": var, "pool": lambda: zb.ed_scalar_mul_host(curve, g, ks[:hm])}
        ts = interleaved(legs)
        scale = {"pool": n / hm}
        say(f"(b) {NAMES[curve]} shared base 2^{lg} items")
        for name in legs:
            say(f"    {name:8s} {fmt(ts[name], scale.get(name, 1.0))}")
        for new, old in (("fixed", "var"), ("fixed", "pool"), ("var", "pool")):
            med, worst = ratio(ts, new, old, scale)
            say(f"    {new} against ({old}): x {med:.2f} median, x {worst:.2f} worst pairing{'  ** LOSS **' if worst < 1.0 else ''}")
            if (new, old) == ("fixed", "var"):
                wins.setdefault(lg, []).append(worst > 1.0)


def scan_leg(be, curve, g, logs):
    width, h, blocks = 3, 0, 1
    for lg in logs:
        n = 1 << lg
        env(ZL_TUNE_ED_DEV_MIN="0", ZL_TUNE_POSEIDON_DEV_MIN="0", ZL_TUNE_ED_FIXED_MIN=None)
        sk = scalars(curve, 1, 3)[0]
        pk, _ = be.ed_scalar_mul(curve, g, sk)
        hd = np.zeros((n, h, 4), dtype=np.uint64)
        tx = scalars(curve, n * blocks * (width - 1), 100 + lg).reshape(n, blocks, width - 1, 4)
        epk, ct, tag, st = be.hybrid_encrypt(curve, None, g, scalars(curve, n, 130 + lg), pk[0], hd, tx)
        assert not st.any()
        pt, ok, st = be.hybrid_decrypt(curve, None, sk, epk, hd, ct, tag)
        assert ok.all() and np.array_equal(pt, tx), "decrypt(encrypt) is not the plaintext"
        hm = min(n, HOST_CAP)
        keys_all, _ = be.ed_scalar_mul(curve, epk, sk)

        def today_mul():
            zb.ed_scalar_mul_host(curve, epk[:hm], sk)

        def today_duplex():
            be.poseidon_duplex_decrypt(curve, None, keys_all, hd, ct, tag)

        legs = {"scan": lambda: be.hybrid_decrypt(curve, None, sk, epk, hd, ct, tag), "host mul": today_mul, "duplex": today_duplex}
        ts = interleaved(legs)
        today = [a * n / hm + b for a, b in zip(ts["host mul"], ts["duplex"])]
        say(f"(c) {NAMES[curve]} scan with one key, (W, H, N) = (3, 0, 1), 2^{lg} ciphertexts")
        say(f"    scan     {fmt(ts['scan'])}")
        say(f"    today    {fmt(today)}  (host multiplications {fmt(ts['host mul'], n / hm)} + duplex {fmt(ts['duplex'])})")
        worst, med = min(today) / max(ts["scan"]), statistics.median(today) / statistics.median(ts["scan"])
        say(f"    scan against (today): x {med:.2f} median, x {worst:.2f} worst pairing{'  ** LOSS **' if worst < 1.0 else ''}")


def devmin_leg(be, curve, g, wins):
    for n in (8, 16, 32, 64, 128, 256):
        env(ZL_TUNE_ED_DEV_MIN="0", ZL_TUNE_ED_FIXED_MIN="0")
        pts, _ = be.ed_scalar_mul(curve, g, scalars(curve, n, 200 + n))
        ks = scalars(curve, n, 300 + n)
        assert np.array_equal(be.ed_scalar_mul(curve, pts, ks)[0], zb.ed_scalar_mul_host(curve, pts, ks)[0])
        ts = interleaved({"device": lambda: be.ed_scalar_mul(curve, pts, ks), "pool": lambda: zb.ed_scalar_mul_host(curve, pts, ks)})
        worst = min(ts["pool"]) / max(ts["device"])
        wins.setdefault(n, []).append(worst > 1.0)
        say(f"devmin {NAMES[curve]} {n:4d} items: device {fmt(ts['device'])}  pool {fmt(ts['pool'])}  "
            f"x {statistics.median(ts['pool']) / statistics.median(ts['device']):.2f} median, x {worst:.2f} worst pairing{'  ** LOSS **' if worst < 1.0 else ''}")


def bound(wins):
    """the smallest size from which every larger measured size won on both curves (None: the largest measured size lost)"""
    best = None
    for k in sorted(wins, reverse=True):
        if not all(wins[k]):
            break
        best = k
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="2^6, 2^10 and 2^14 only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edwards_bench.log"))
    args = ap.parse_args()
    be = Backend(0)
    say(be.describe())
    props = torch.cuda.get_device_properties(0)
    SATURATED[0] = props.multi_processor_count * 4 * 64
    say(f"lanes at one wave per SIMD: {SATURATED[0]}; host pool legs on {os.cpu_count()} logical CPUs (OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')})")
    logs = (6, 10, 14) if args.quick else tuple(range(6, 19))
    fixed_wins, dev_wins = {}, {}
    try:
        for curve in (ZL_BLS12_381, ZL_BN254):
            g = a_point(curve)
            variable_leg(be, curve, g, logs)
            shared_leg(be, curve, g, logs, fixed_wins)
            scan_leg(be, curve, g, logs)
            devmin_leg(be, curve, g, dev_wins)
        b = bound(dev_wins)
        say(f"ZL_TUNE_ED_DEV_MIN: the device won every repetition on both curves from {b} items" if b else "ZL_TUNE_ED_DEV_MIN: the device lost at the largest size measured")
        b = bound(fixed_wins)
        say(f"ZL_TUNE_ED_FIXED_MIN: the fixed-base kernel won every repetition on both curves from 2^{b} items" if b else
            "ZL_TUNE_ED_FIXED_MIN: the fixed-base kernel lost at the largest size measured")
    finally:
        be.close()
    with open(args.out, "w") as f:  # only a complete run replaces the log
        f.write("\n".join(LOG) + "\n")


if __name__ == "__main__":
    main()
