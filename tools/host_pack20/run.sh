#!/bin/bash
# ASan + UBSan run of the 20-bit unit-block entries' pack / unpack arithmetic (include/mgx/pack20.hpp) compiled for the HOST:
# a stand-alone program with its own main, nothing preloaded, no HIP call, no GPU.
# usage: bash tools/host_pack20/run.sh        (exits non-zero on a sanitizer finding or a failed expectation)
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/../.." && pwd)"
WORK=$(mktemp -d /tmp/mgx_host_pack20.XXXXXX)
trap 'rm -rf "$WORK"' EXIT
timeout 600 ${HIPCC:-/opt/rocm/bin/hipcc} --offload-arch=gfx950 --cuda-host-only -O1 -g -std=c++17 -Wno-unused-value -I"$ROOT/include" \
    -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer \
    -fsanitize=address,undefined "$ROOT/tools/host_pack20/host_pack20.hip" -o "$WORK/host_pack20"
ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=print_stacktrace=1 timeout 600 "$WORK/host_pack20"
