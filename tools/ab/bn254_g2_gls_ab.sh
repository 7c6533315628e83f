#!/bin/bash
# Interleaved A/B of the BN254 G2 endomorphism split against the parent commit's library (log: profiles/bn254_g2_gls_ab.log).
#   bash tools/ab/bn254_g2_gls_ab.sh > profiles/bn254_g2_gls_ab.log
# "parent": openzl_amd/libzl_backend.parent.so, the library built from the commit before the split (python -m openzl_amd.build in a worktree of that commit,
# copied here under that name); it plans plain 254-bit windows.  "open": openzl_amd/libzl_backend.open.so, this tree built without the size gate of MsmJob::plan,
#   ZL_BUILD_TAG=open ZL_EXTRA_FLAGS="-DZL_GLS_HOLE_LO_LOG=0 -DZL_GLS_HOLE_HI_LOG=0 -DZL_GLS_END_LOG=32" python -m openzl_amd.build
# and, for the MSM sizes, run with ZL_TUNE_GLV_MAX_LOG=20, so every size takes the split (the proofs keep the default 19 on both sides: the knob moves their G1
# MSMs too).  Both are loaded through ZL_BACKEND_LIB: same Python, same tools on both sides.
# Three runs of each side, alternating, one process per run; then BN254 Poseidon-chain proofs of 235 / 14 977 / 958 465 constraints (k = 1 / 64 / 4096).
# A failing step ends the script.
set -e -o pipefail
cd "$(dirname "$0")/../.."
PARENT_LIB=$PWD/openzl_amd/libzl_backend.parent.so
OPEN_LIB=$PWD/openzl_amd/libzl_backend.open.so
for lib in "$PARENT_LIB" "$OPEN_LIB"; do
    [ -f "$lib" ] || { echo "$lib: build it first (see the head of this script)" >&2; exit 2; }
done
for run in 1 2 3; do
    timeout -k 10 150 env ZL_BACKEND_LIB="$PARENT_LIB" python tools/msm_g2_ab.py parent
    timeout -k 10 150 env ZL_BACKEND_LIB="$OPEN_LIB" ZL_TUNE_GLV_MAX_LOG=20 python tools/msm_g2_ab.py open
done
for run in 1 2; do
    for k in 1 64 4096; do
        timeout -k 10 200 env ZL_BACKEND_LIB="$PARENT_LIB" CURVE=bn254 ITERS=${ITERS:-8} python tools/g16_one.py $k | sed -n 's/^prove k=/[parent] prove k=/p'
        timeout -k 10 200 env ZL_BACKEND_LIB="$OPEN_LIB" CURVE=bn254 ITERS=${ITERS:-8} python tools/g16_one.py $k | sed -n 's/^prove k=/[open] prove k=/p'
    done
done
# the comparison table: python tools/msm_g2_ab.py --digest profiles/bn254_g2_gls_ab.log
