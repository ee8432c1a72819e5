#!/bin/bash
# Diagnostic build of the HIP library with per-workgroup phase stamps (never used by the product path):
#   tools/build_stamps.sh  ->  build/stamps/libmindpose_hip.so   (use with MINDPOSE_HIP_LIB=...)
# MP_STAMPS_FLAGS picks the stamp sets (default: all three).  The stamps cost registers, and the Makefile's scratch gates hold for
# this build too: for tools/bench_wino.py build the conv stamps alone (MP_STAMPS_FLAGS=-DMP_CONV_STAMPS=1).
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
mkdir -p "$ROOT/build/stamps"
cp "$ROOT"/mindpose_amd/csrc/*.hip "$ROOT"/mindpose_amd/csrc/*.h "$ROOT"/mindpose_amd/csrc/Makefile "$ROOT/build/stamps/"
make -C "$ROOT/build/stamps" -j8 EXTRA="${MP_STAMPS_FLAGS:--DMP_CONV_STAMPS=1 -DMP_BLOCK_STAMPS=1 -DMP_WS_STAMPS=1} $MP_STAMPS_EXTRA"
