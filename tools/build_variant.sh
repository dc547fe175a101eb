#!/bin/bash
# One A/B variant of the HIP library: lines_kernel.hip, far_kernel.hip and api.hip recompiled with extra flags, the other objects taken from
# the shipped build (monortm_amd/lib/obj/, built by __graft_entry__.build()).
#   tools/build_variant.sh NAME [-DFLAG ...]      -> build_dbg/libmonortm_hip_NAME.so   (git-ignored, travels with gpurun)
# Select it with MONORTM_HIP_LIB=$PWD/build_dbg/libmonortm_hip_NAME.so (monortm_amd/api.py), or through tools/ab_libs.sh.
set -e
NAME=$1; shift
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
CSRC=$ROOT/monortm_amd/csrc
OBJ=$ROOT/monortm_amd/lib/obj
OUT=$ROOT/build_dbg
mkdir -p $OUT/obj_$NAME
CF="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value -Wno-pass-failed -Wno-unused-const-variable"
/opt/rocm/bin/hipcc $CF -mllvm -disable-machine-licm -DMONORTM_EXPERIMENT=1 "$@" -c $CSRC/lines_kernel.hip -o $OUT/obj_$NAME/lines_kernel.o &
/opt/rocm/bin/hipcc $CF -DMONORTM_EXPERIMENT=1 "$@" -c $CSRC/api.hip -o $OUT/obj_$NAME/api.o &
/opt/rocm/bin/hipcc $CF -DMONORTM_EXPERIMENT=1 "$@" -c $CSRC/far_kernel.hip -o $OUT/obj_$NAME/far_kernel.o &
wait
# every other object of the shipped build, whatever _build.py's HIP_SOURCES lists by now
REST=$(ls $OBJ/*.o | grep -v -e /lines_kernel.o -e /api.o -e /far_kernel.o)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT/libmonortm_hip_$NAME.so $OUT/obj_$NAME/lines_kernel.o $OUT/obj_$NAME/api.o $OUT/obj_$NAME/far_kernel.o $REST
ls -la $OUT/libmonortm_hip_$NAME.so
