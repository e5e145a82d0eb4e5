#!/bin/bash
# Build libart.so with extra compile flags into variants/libart_<name>.so (A/B experiments;
# bench.py / tests pick it up through ART_LIB=variants/libart_<name>.so).
#   tools/build_variant.sh <name> [-DFLAG ...]
set -euo pipefail
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
pkg=$root/audio-raytracer_amd
tmp=$(mktemp -d)
mkdir -p "$root/variants"
flags=(--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden "$@")
# the shipped build's scheduler (audio-raytracer_amd/Makefile SCHED; ART_SCHED= for the default one)
sched=(${ART_SCHED--mllvm -amdgpu-sched-strategy=max-ilp})
# every source of the directory, as the Makefile lists them; art_bvh.hip keeps the default scheduler
for f in "$pkg"/csrc/*.hip; do
  b=$(basename "$f" .hip)
  if [ "$b" = art_bvh ]; then hipcc "${flags[@]}" -c "$f" -o "$tmp/$b.o" &
  else hipcc "${flags[@]}" "${sched[@]}" -c "$f" -o "$tmp/$b.o" & fi
done
for f in "$pkg"/csrc/*.cpp; do
  hipcc "${flags[@]}" "${sched[@]}" -x hip -c "$f" -o "$tmp/$(basename "$f" .cpp).o" &
done
wait
hipcc --offload-arch=gfx950 -shared -fPIC -rdynamic -o "$root/variants/libart_$name.so" "$tmp"/*.o
rm -rf "$tmp"
echo "variants/libart_$name.so"
