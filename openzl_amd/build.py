"""Build libzl_backend.so (HIP, gfx950) in-tree with hipcc.  Incremental: objects are rebuilt only when a source or
header they include changed.  Used by __graft_entry__.build(); `python -m openzl_amd.build` works too."""
from __future__ import annotations

import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
ROOT = os.path.dirname(HERE)
LIB = os.path.join(HERE, "libzl_backend.so")
ARCH = "gfx950"
FLAGS = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unused-result"]
FLAGS += [f for f in os.environ.get("ZL_EXTRA_FLAGS", "").split() if f]
GROUPS = ["BlsG1", "BnG1", "BlsG2", "BnG2"]
# Developer A/B builds: ZL_BUILD_TAG=x writes objects *.x.o and libzl_backend.x.so beside the product build (load it with ZL_BACKEND_LIB, tools/ab/*.sh)
TAG = os.environ.get("ZL_BUILD_TAG", "")
if TAG:
    LIB = os.path.join(HERE, f"libzl_backend.{TAG}.so")
_LLVM = "/opt/rocm/lib/llvm/bin"
_INC = re.compile(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', re.M)


def _deps(src: str) -> list[str]:
    """Every file `src` reaches through quoted #include lines (recursively, whatever the preprocessor conditions say: device-only
    includes count too).  Derived from the sources on every build, so a new header can never be forgotten in a hand-kept list
    (round 3's zl_quad.h / zl_pool.h were)."""
    seen, todo = [], [os.path.normpath(src)]
    while todo:
        f = todo.pop()
        if f in seen or not os.path.exists(f):
            continue
        seen.append(f)
        with open(f, encoding="utf-8", errors="replace") as fh:
            for inc in _INC.findall(fh.read()):
                todo.append(os.path.normpath(os.path.join(os.path.dirname(f), inc)))
    return sorted(seen)


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def _digest(paths, extra="") -> str:
    h = hashlib.sha256(extra.encode())
    for p in paths:
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def _units():
    units = [("zl_capi", "zl_capi.hip", []), ("zl_ntt", "zl_ntt.hip", ["-DZL_INLINE_MUL"]), ("zl_groth16", "zl_groth16.hip", []), ("zl_host", "zl_host.hip", []), ("zl_verify", "zl_verify.hip", []), ("zl_testhooks", "zl_testhooks.hip", []), ("zl_multi", "zl_multi.hip", []),
             ("zl_msm_sort", "zl_msm_sort.hip", []),  # the curve-independent sort kernels of the MSM: once, not per group
             ("zl_pairing_dev_bls", "zl_pairing_dev.hip", ["-DZL_PAIR_CURVE=1"]), ("zl_pairing_dev_bn", "zl_pairing_dev.hip", ["-DZL_PAIR_CURVE=2"]),  # device Miller loops, once per curve
             ("zl_decode_dev_bls", "zl_decode_dev.hip", ["-DZL_DECODE_CURVE=1"]), ("zl_decode_dev_bn", "zl_decode_dev.hip", ["-DZL_DECODE_CURVE=2"]),  # device point / proof decoders, once per curve
             ("zl_poseidon_dev", "zl_poseidon_dev.hip", ["-DZL_INLINE_MUL_DEVICE"]),  # batched Poseidon, both curves in one unit; the multiplier inlined in the round loop
             ("zl_edwards_dev", "zl_edwards_dev.hip", ["-DZL_INLINE_MUL_DEVICE"])]  # embedded-curve scalar multiplication and hybrid encryption, both curves in one unit
    for g in GROUPS:
        # G1 device code inlines the multiplier: -4.5 % on the accumulate kernel vs the out-of-line call (host code keeps the call).
        extra = ["-DZL_INLINE_MUL_DEVICE"] if g.endswith("G1") else []
        if g == "BlsG1":
            # three waves per SIMD (<= 168 registers): what the accumulation kernel needs anyway (162); without the cap the compiler spreads to 185 = two waves
            extra = extra + ["-DZL_ACC_WAVES=3"]
        # three units per group: the host side + light kernels, the accumulation kernels, the merge / reduction kernels (zl_msm.hip's header);
        # a fourth for the multi-vector MSM (zl_msm_multi.hip)
        for part in ("zl_msm", "zl_msm_acc", "zl_msm_tail", "zl_msm_multi"):
            units.append((f"{part}_{g}", part + ".hip", [f"-DZL_G={g}"] + extra))
    return [u for u in units if os.path.exists(os.path.join(CSRC, u[1]))]


def build(verbose: bool = True, jobs: int | None = None) -> str:
    params = os.path.join(CSRC, "zl_params.h")
    gen = os.path.join(CSRC, "gen_params.py")
    if not os.path.exists(params) or os.path.getmtime(params) < os.path.getmtime(gen):
        subprocess.check_call([sys.executable, gen])
    # the generated product scans (committed, like zl_params.h): regenerate when their generator is newer, so that an edit of gen_mul*.py can never
    # leave a stale header behind; the object digests then see the new text
    for g, outs in (("gen_mul28.py", ("zl_mul28_gfx950.h", "zl_mul28r_gfx950.h", "zl_mul29r_gfx950.h")), ("gen_mul.py", ("zl_mul_gfx950.h",))):
        gp = os.path.join(CSRC, g)
        if os.path.exists(gp) and any(not os.path.exists(os.path.join(CSRC, o)) or os.path.getmtime(os.path.join(CSRC, o)) < os.path.getmtime(gp) for o in outs):
            subprocess.check_call([sys.executable, gp], stdout=subprocess.DEVNULL)
    todo, objs = [], []
    for name, src, defs in _units():
        obj = os.path.join(CSRC, name + (f".{TAG}" if TAG else "") + ".o")
        stamp = obj + ".sha"
        d = _digest(_deps(os.path.join(CSRC, src)), " ".join(FLAGS + defs))
        objs.append(obj)
        if os.path.exists(obj) and os.path.exists(stamp) and open(stamp).read() == d:
            continue
        todo.append((name, src, defs, obj, stamp, d))

    def compile_one(t):
        name, src, defs, obj, stamp, d = t
        cmd = [_hipcc()] + FLAGS + defs + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print("[build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        with open(stamp, "w") as f:
            f.write(d)

    if todo:
        with ThreadPoolExecutor(max_workers=jobs or min(8, os.cpu_count() or 1)) as ex:
            list(ex.map(compile_one, todo))
    if todo or not os.path.exists(LIB):
        cmd = [_hipcc(), "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB] + objs + ["-ldl"]  # RCCL is dlopen'ed on first multi-GPU use
        if verbose:
            print("[build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return LIB


# ---- sanitizer build of the HOST side (VERDICT r4 "next" item 7) -----------------------------------------------------------------------------
# zl_host.hip holds every parser of untrusted bytes (zl_groth16_keys_from_bytes, zl_point_from_bytes*: zl_serialize.h) and the R1CS / Poseidon / Groth16 mirror;
# zl_verify.hip the host pairing (zl_pairing.h) and verification; zl_capi.hip the handle and argument checks.  `python -m openzl_amd.build --host-asan` compiles the
# HOST half of those three units with -fsanitize=address,undefined (device code and every other unit: the product objects) and links libzl_backend.asan.so against the shared ASan
# runtime; tests/test_sanitizers.py runs the serialisation / pairing / host-mirror tests (and, on a GPU box, the key-wire corruption fuzz) against it with
# the runtime preloaded.  Any report aborts the process (-fno-sanitize-recover=all).
ASAN_UNITS = ("zl_host", "zl_verify", "zl_capi")
ASAN_FLAGS = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-Xarch_host", "-fno-omit-frame-pointer", "-Xarch_host", "-g"]
ASAN_LIB = os.path.join(HERE, "libzl_backend.asan.so")


def asan_runtime() -> str:
    out = subprocess.check_output([_hipcc(), "-print-file-name=libclang_rt.asan-x86_64.so"], text=True).strip()
    if not os.path.isabs(out) or not os.path.exists(out):
        cands = [os.path.join(d, f) for d, _, fs in os.walk(os.path.join(_LLVM, "..", "lib", "clang")) for f in fs if f == "libclang_rt.asan-x86_64.so"]
        if not cands:
            raise RuntimeError("no shared ASan runtime (libclang_rt.asan-x86_64.so) beside hipcc")
        out = os.path.normpath(cands[0])
    return out


def build_host_asan(verbose: bool = True) -> str:
    build(verbose=verbose)  # the product objects of every other unit
    objs, todo = [], []
    for name, src, defs in _units():
        if name not in ASAN_UNITS:
            objs.append(os.path.join(CSRC, name + ".o"))
            continue
        obj = os.path.join(CSRC, name + ".asan.o")
        stamp = obj + ".sha"
        d = _digest(_deps(os.path.join(CSRC, src)), " ".join(FLAGS + defs + ASAN_FLAGS))
        objs.append(obj)
        if not (os.path.exists(obj) and os.path.exists(stamp) and open(stamp).read() == d):
            todo.append((name, src, defs, obj, stamp, d))

    def one(t):
        name, src, defs, obj, stamp, d = t
        cmd = [_hipcc()] + FLAGS + defs + ASAN_FLAGS + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print("[build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        open(stamp, "w").write(d)

    if todo:
        with ThreadPoolExecutor(max_workers=2) as ex:
            list(ex.map(one, todo))
    if todo or not os.path.exists(ASAN_LIB) or os.path.getmtime(ASAN_LIB) < os.path.getmtime(LIB):
        cmd = [_hipcc(), "--offload-arch=" + ARCH, "-shared", "-fPIC", "-fsanitize=address,undefined", "-shared-libasan", "-o", ASAN_LIB] + objs + ["-ldl"]
        if verbose:
            print("[build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return ASAN_LIB


if __name__ == "__main__":
    print(build_host_asan() if "--host-asan" in sys.argv else build())
