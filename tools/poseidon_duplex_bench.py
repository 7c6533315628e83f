"""Throughput of the batched Poseidon duplex cipher (zl_poseidon_duplex_encrypt_batch), both curves, widths 3 and 6.

  python tools/poseidon_duplex_bench.py [--quick] [--out profiles/poseidon_duplex_bench.log]

Every leg is checked before it is timed, the legs of a line are interleaved in one process, five repetitions after one warm-up round; a line gives the median,
[min .. max], and ratios on the WORST pairing of repetitions (slowest run of the new call against the fastest run of the other side).

  sizes     2^6 / 2^10 / 2^14 / 2^18 messages, shapes (K, H, N) = (2, 0, 1) and (2, 0, 8):
            (dev)     the new call on device operands (zl_poseidon_duplex_encrypt_batch_dev, in place);
            (hostptr) the new call on host operands, copies included;
            (a pool)  the same call with ctx == NULL: the host mirror over the host pool, the loop a caller writes today.  Timed over at most 2^12 messages and
                      scaled (equal, independent messages);
            (b comp)  the best composition of existing entry points: SB + N calls of zl_poseidon_permute_batch(_w) on host states with the absorb step -- the
                      addition mod r on four 64-bit words -- in numpy between them.
            Derived: the expected time of the device-operand leg, (SB + N) x one permutation's latency (0.42 ms at width 3, 1.31 ms at width 6: DESIGN.md 4.7),
            times lanes / (CUs x 4 x 64) once every SIMD holds more than one wave, and the deviation from it.
  devmin    host-pointer calls of 32 / 64 / 128 messages on the device against the host pool: ZL_TUNE_POSEIDON_DEV_MIN (64) is shared with the other entry
            points; a loss at 64 is reported as a loss.
Checks: the device ciphertexts and tags against the ctx == NULL call (the first 1 024 messages) and against composition (b) (all of them)."""
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
LATENCY_MS = {3: 0.42, 4: 0.64, 5: 0.96, 6: 1.31}  # one permutation, one lane per SIMD slot
REPS = 5
HOST_CAP = 1 << 12
LOG = []


def say(line):
    print(line, flush=True)
    LOG.append(line)


def elems(shape, seed):
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 2 ** 63, size=tuple(shape) + (4,), dtype=np.uint64)
    out[..., 3] &= np.uint64((1 << 59) - 1)  # < 2^251 < r on both curves
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


def addmod(a, b, r):
    """(a + b) mod r on (..., 4) uint64 words, a, b < r < 2^255"""
    rw = [np.uint64((r >> (64 * i)) & (2 ** 64 - 1)) for i in range(4)]
    s = np.empty_like(a)
    c = np.zeros(a.shape[:-1], dtype=np.uint64)
    for i in range(4):
        t = a[..., i] + b[..., i]
        c1 = t < a[..., i]
        t2 = t + c
        s[..., i] = t2
        c = (c1 | (t2 < t)).astype(np.uint64)
    d = np.empty_like(s)
    bor = np.zeros(a.shape[:-1], dtype=np.uint64)
    for i in range(4):
        t = s[..., i] - rw[i]
        b1 = s[..., i] < rw[i]
        d[..., i] = t - bor
        bor = (b1 | (t < bor)).astype(np.uint64)
    return np.where((bor == 0)[..., None], d, s)


def composed(be, curve, width, init, keys, texts):
    """encryption out of existing entry points: permute_batch per block, the absorb in numpy (header_len 0: one all-zero header block)"""
    n, blocks, rate = texts.shape[0], texts.shape[1], width - 1
    r = MODULUS[curve]
    st = np.ascontiguousarray(np.broadcast_to(init, (n, width, 4))).copy()
    k = keys.shape[1]
    for b in range(k // rate + 1):
        part = keys[:, b * rate:(b + 1) * rate]
        if part.shape[1]:
            st[:, 1:1 + part.shape[1]] = addmod(st[:, 1:1 + part.shape[1]], part, r)
        st = be.poseidon_permute_batch(curve, st)
    st = be.poseidon_permute_batch(curve, st)
    ct = np.empty_like(texts)
    for j in range(blocks):
        st[:, 1:] = addmod(st[:, 1:], texts[:, j], r)
        ct[:, j] = st[:, 1:]
        st = be.poseidon_permute_batch(curve, st)
    return ct, st[:, 1].copy()


def dev_tensor(a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    return t


def data(width, shape, n, seed):
    k, h, blocks = shape
    return elems((width,), seed), elems((n, k), seed + 1), np.zeros((n, h, 4), dtype=np.uint64), elems((n, blocks, width - 1), seed + 2)


def sizes_leg(be, curve, width, shape, logs):
    k, h, blocks = shape
    perms = zb.poseidon_duplex_permutations(width, k, h, blocks)
    for lg in logs:
        n = 1 << lg
        init, keys, headers, texts = data(width, shape, n, 1000 * width + lg)
        os.environ["ZL_TUNE_POSEIDON_DEV_MIN"] = "0"
        ct, tags = be.poseidon_duplex_encrypt(curve, init, keys, headers, texts)
        m = min(n, 1024)
        ct_h, tags_h = zb.poseidon_duplex_encrypt_host(curve, init, keys[:m], headers[:m], texts[:m])
        assert np.array_equal(ct_h, ct[:m]) and np.array_equal(tags_h, tags[:m]), "device and host mirror differ"
        ct_c, tags_c = composed(be, curve, width, init, keys, texts)
        assert np.array_equal(ct_c, ct) and np.array_equal(tags_c, tags), "the composition of existing calls differs from the new call"
        d_k, d_t, d_g = dev_tensor(keys), dev_tensor(texts), dev_tensor(np.zeros((n, 4), dtype=np.uint64))
        hm = min(n, HOST_CAP)
        hk, hh, ht = keys[:hm], headers[:hm], texts[:hm]
        legs = {
            "dev": lambda: be.poseidon_duplex_encrypt_dev(curve, width, init, d_k.data_ptr(), k, 0, h, d_t.data_ptr(), blocks, n, d_t.data_ptr(), d_g.data_ptr()),
            "hostptr": lambda: be.poseidon_duplex_encrypt(curve, init, keys, headers, texts),
            "a pool": lambda: zb.poseidon_duplex_encrypt_host(curve, init, hk, hh, ht),
            "b comp": lambda: composed(be, curve, width, init, keys, texts),
        }
        ts = interleaved(legs)
        scale = {"a pool": n / hm}
        say(f"{NAMES[curve]} W={width} (K,H,N)={shape} 2^{lg} messages, {perms} permutations each")
        for name in legs:
            say(f"    {name:8s} {fmt(ts[name], scale.get(name, 1.0))}")
        for new in ("dev", "hostptr"):
            for old in ("a pool", "b comp"):
                worst = min(ts[old]) * scale.get(old, 1.0) / max(ts[new])
                med = statistics.median(ts[old]) * scale.get(old, 1.0) / statistics.median(ts[new])
                say(f"    {new} against ({old}): x {med:.2f} median, x {worst:.2f} worst pairing{'  ** LOSS **' if worst < 1.0 else ''}")
        fill = max(1.0, n / SATURATED[0])
        expect = perms * LATENCY_MS[width] * fill
        got = statistics.median(ts["dev"]) * 1e3
        say(f"    expected (SB + N) x latency x {fill:g} (lanes over one wave per SIMD) = {expect:.3f} ms, dev measured {got:.3f} ms: {100.0 * (got - expect) / expect:+.1f} %")


SATURATED = [0]


def devmin_leg(be, curve, width, shape):
    for n in (32, 64, 128):
        init, keys, headers, texts = data(width, shape, n, 77 + n)
        os.environ["ZL_TUNE_POSEIDON_DEV_MIN"] = "0"
        assert np.array_equal(be.poseidon_duplex_encrypt(curve, init, keys, headers, texts)[0], zb.poseidon_duplex_encrypt_host(curve, init, keys, headers, texts)[0])
        ts = interleaved({"device": lambda: be.poseidon_duplex_encrypt(curve, init, keys, headers, texts),
                          "pool": lambda: zb.poseidon_duplex_encrypt_host(curve, init, keys, headers, texts)})
        worst = min(ts["pool"]) / max(ts["device"])
        say(f"devmin {NAMES[curve]} W={width} (K,H,N)={shape} {n:4d} messages: device {fmt(ts['device'])}  pool {fmt(ts['pool'])}  "
            f"x {statistics.median(ts['pool']) / statistics.median(ts['device']):.2f} median, x {worst:.2f} worst pairing{'  ** LOSS **' if worst < 1.0 else ''}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="2^6 and 2^10 only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poseidon_duplex_bench.log"))
    args = ap.parse_args()
    be = Backend(0)
    say(be.describe())
    props = torch.cuda.get_device_properties(0)
    # the permutation is bound by the integer VALU: one wave per SIMD already fills it, so beyond CUs x 4 SIMDs x 64 lanes the time grows with the count
    SATURATED[0] = props.multi_processor_count * 4 * 64
    say(f"lanes at one wave per SIMD: {SATURATED[0]}")
    logs = (6, 10) if args.quick else (6, 10, 14, 18)
    try:
        for curve in (ZL_BLS12_381, ZL_BN254):
            for width in (3, 6):
                for shape in ((2, 0, 1), (2, 0, 8)):
                    sizes_leg(be, curve, width, shape, logs)
        for curve in (ZL_BLS12_381, ZL_BN254):
            for width in (3, 6):
                devmin_leg(be, curve, width, (2, 0, 1))
    finally:
        be.close()
        with open(args.out, "w") as f:
            f.write("\n".join(LOG) + "\n")


if __name__ == "__main__":
    main()
