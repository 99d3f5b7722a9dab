#!/bin/bash
# Builds tools/scene_digest.cpp with the library's host flags against the host sources under CSRC
# (default: this tree's; point it at another checkout's csrc to compare two commits) and prints
# the digests of every preset, USD input and error path (CPU only):
#   bash tools/scene_digest.sh > new.txt; CSRC=/path/to/parent/csrc bash tools/scene_digest.sh > parent.txt
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
C=${CSRC:-$R/metal4-raytracing_amd/csrc}
B=$(mktemp -d /tmp/scene_digest.XXXXXX)
trap 'rm -rf "$B"' EXIT
g++ -O3 -std=c++17 -ffp-contract=off -fno-fast-math -Wall -I$R/include -o $B/scene_digest $R/tools/scene_digest.cpp \
    $C/rt_scene*.cpp $C/rt_usd*.cpp $C/rt_bvh.cpp $C/rt_texture.cpp -lz -lpthread
# assets/ is what build() of __graft_entry__.py unpacks from tests/golden/scene_data
[ -f $R/assets/sphere.obj ] || { echo "no $R/assets: run build() of __graft_entry__.py first" >&2; exit 1; }
python3 $R/tools/scene_digest_inputs.py $B/inputs
ln -s $R/assets $B/assets
cd $B && ./scene_digest assets inputs   # relative paths: the error texts name them
