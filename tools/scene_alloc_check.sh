#!/bin/bash
# Builds tools/scene_alloc_check.cpp with the host sources under CSRC (default: this tree's), the
# translation units in parallel, and runs it (CPU only).  SANITIZE=1 builds it under AddressSanitizer
# + UBSan with leak detection (a few times slower to build):
#   bash tools/scene_alloc_check.sh; SANITIZE=1 bash tools/scene_alloc_check.sh
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
C=${CSRC:-$R/metal4-raytracing_amd/csrc}
B=$(mktemp -d /tmp/scene_alloc_build.XXXXXX)
trap 'rm -rf "$B"' EXIT
FLAGS="-std=c++17 -O0 -ffp-contract=off -I$R/include"
[ -z "$SANITIZE" ] || FLAGS="$FLAGS -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined"
ls $R/tools/scene_alloc_check.cpp $C/rt_scene*.cpp $C/rt_usd*.cpp $C/rt_texture.cpp |
    xargs -P 12 -I{} sh -c "g++ $FLAGS -c {} -o $B/\$(basename {} .cpp).o"
g++ $FLAGS -o $B/scene_alloc_check $B/*.o -lz -lpthread
ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1 $B/scene_alloc_check
