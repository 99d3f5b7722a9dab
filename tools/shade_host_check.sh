#!/bin/bash
# Builds tools/shade_host_check.cpp with csrc/rt_scatter_host.cpp (the host side of the shading
# query: scatter_eval compiled for the host) under AddressSanitizer + UBSan and runs it (CPU only;
# the program makes no device call).  hipcc compiles the host side only: the sources share headers
# with the kernels.  SANITIZE=0 builds it plain.
#   bash tools/shade_host_check.sh
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
C=${CSRC:-$R/metal4-raytracing_amd/csrc}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
B=$(mktemp -d /tmp/shade_host_build.XXXXXX)
trap 'rm -rf "$B"' EXIT
FLAGS="-x hip --offload-host-only -std=c++17 -O1 -g -ffp-contract=off -fno-fast-math"
[ "$SANITIZE" = 0 ] || FLAGS="$FLAGS -fsanitize=address,undefined -fno-sanitize-recover=undefined"
$HIPCC $FLAGS -c $R/tools/shade_host_check.cpp -o $B/check.o &
$HIPCC $FLAGS -c $C/rt_scatter_host.cpp -o $B/scatter_host.o
wait %1
LINK=""
[ "$SANITIZE" = 0 ] || LINK="-fsanitize=address,undefined"
$HIPCC $LINK -o $B/shade_host_check $B/check.o $B/scatter_host.o
ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1 $B/shade_host_check
