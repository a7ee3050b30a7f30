#!/bin/bash
# A/B builds of libdlwp_hip.so with extra hipcc flags for ONE source: tools/ab_build.sh <tag> <file.hip> [-D... ...]
# -> dlwp_benchmark_amd/ab/lib_<tag>.so (git-ignored, travels to the GPU box); select with DLWP_HIP_LIB=<path>.
# The source is compiled by csrc/Makefile itself (BUILD= / EXTRA=), so it gets exactly the flags of the shipped build,
# the per-file ones included, plus the extra ones; every other object is the shipped build's.
set -e
tag=$1; src=$2; shift; shift
base=${src%.hip}
cd "$(dirname "$0")/../dlwp_benchmark_amd/csrc"
[ -f "$base.hip" ] || { echo "usage: tools/ab_build.sh <tag> <file.hip> [extra hipcc flags]" >&2; exit 2; }
make -s -j8 >/dev/null
rm -rf build/ab_$tag
make -s BUILD=build/ab_$tag EXTRA="$*" build/ab_$tag/$base.o
mkdir -p ../ab
objs=$(ls build/*.o | grep -v "build/$base.o")
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o ../ab/lib_$tag.so build/ab_$tag/$base.o $objs -L/opt/rocm/lib -lhipfft
echo built dlwp_benchmark_amd/ab/lib_$tag.so
