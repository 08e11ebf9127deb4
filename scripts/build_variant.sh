#!/bin/bash
# Development tool: build scripts/variants/libthesia_amd_<tag>.so (outside the package directory) with extra -D flags (A/B on one GPU box:
# THESIA_AMD_LIB=scripts/variants/libthesia_amd_<tag>.so python scripts/bench_stft.py).
# usage: scripts/build_variant.sh <tag> [flags...]     (run after __graft_entry__.build())
# By default only kernels_stft.hip is recompiled; VARIANT_SOURCES="kernels_image.hip api.hip" picks others.
# Only the named sources see the flags: an image-stage variant that changes how jobs are cut (-DTH_FUSED_FB, -DTH_RASTER_QPB, ...) must
# name batch_plan.cpp as well, where the planners count blocks with the same constants: VARIANT_SOURCES="kernels_image.hip batch_plan.cpp".
# The link list and each source's own flags come from __graft_entry__ (SOURCES, EXTRA_FLAGS): the variant links what the product does.
set -e
tag=$1; shift
root="$(cd "$(dirname "$0")/.." && pwd)"
cd "$root/thesia_amd/csrc"
srcs=${VARIANT_SOURCES:-kernels_stft.hip kernels_stft_w1024.hip kernels_stft_w2048.hip kernels_stft_w4096.hip}   # (kernels_stft.hip is four translation units)
obj=../../build/obj   # __graft_entry__.build()'s object cache
# one line per source of the product library: "<source> <its extra flags>"
sources=$(cd "$root" && python3 -c 'import __graft_entry__ as g
for s in g.SOURCES: print(s, *g.EXTRA_FLAGS.get(s, []))')
objs="" pids=""
while read -r f extra; do
  if [[ " $srcs " == *" $f "* ]]; then
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden $extra "$@" -c $f -o $obj/${f}_$tag.o &
    pids="$pids $!"
    objs="$objs $obj/${f}_$tag.o"
  else
    objs="$objs $obj/$f.o"
  fi
done <<< "$sources"
for pid in $pids; do wait $pid; done   # (a failed compile stops the script: no link against a stale object)
out=${VARIANT_DIR:-../../scripts/variants}; mkdir -p $out && hipcc --offload-arch=gfx950 -shared -fPIC -o $out/libthesia_amd_$tag.so $objs
echo built $out/libthesia_amd_$tag.so
