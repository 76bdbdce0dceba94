#!/bin/bash
# dev: a development build of the library with extra macros for ONE source file, for A/B runs on the GPU box through MSCOMP_AMD_LIB
# (hipcc cross-compiles here; build/ travels with the snapshot).   usage: tools/dev/build_variant.sh <name> <source stem> "<-D flags>" [source file]
set -e
R=$(cd "$(dirname "$0")/../.." && pwd)
C=$R/ms_compress_amd/csrc
mkdir -p $R/build
make -C $C -j8 > /dev/null
SRC=${4:-$C/$2.hip}                                             # (4th argument: another text of that source file, e.g. the parent's)
OBJS=$(sed -n 's/^OBJS *= *//p' $C/Makefile)                  # (the Makefile's own list)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-exceptions -Wno-unused-function $3 -I$C -c $SRC -o $R/build/$2_$1.o
(cd $C && /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $R/build/libmscomp_amd_$1.so ${OBJS/$2.o/$R/build/$2_$1.o})
echo built build/libmscomp_amd_$1.so
