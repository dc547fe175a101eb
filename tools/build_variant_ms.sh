#!/bin/bash
# One A/B variant of the HIP library for lines_ms_kernel: lines_ms_kernel.hip and api.hip recompiled with extra flags (experiment
# switches allowed), the other objects from the shipped build (monortm_amd/lib/obj/).
#   tools/build_variant_ms.sh NAME [-DFLAG ...]   -> build_dbg/libmonortm_hip_NAME.so   (git-ignored, travels with gpurun)
# For TIMING an experiment build add -DMONORTM_NO_PLAN_STATS: the chunk-plan counters (MONORTM_MS_PLAN_STATS) are two atomicAdd on one
# line per chunk and take the kernel from 0.85 to 4.2 ms on configs[3].  MONORTM_MS_ABLATE values: device_common.hpp (MsArgs::ablate);
# 7 = the completion of a molecule run without its loads and without the sum over the molecules (lines_ms_kernel.hip).
set -e
NAME=$1; shift
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
CSRC=$ROOT/monortm_amd/csrc
OBJ=$ROOT/monortm_amd/lib/obj
OUT=$ROOT/build_dbg
mkdir -p $OUT/obj_$NAME
CF="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value -Wno-pass-failed -Wno-unused-const-variable"
/opt/rocm/bin/hipcc $CF -mllvm -disable-machine-licm -DMONORTM_EXPERIMENT=1 "$@" -c $CSRC/lines_ms_kernel.hip -o $OUT/obj_$NAME/lines_ms_kernel.o &
/opt/rocm/bin/hipcc $CF -DMONORTM_EXPERIMENT=1 "$@" -c $CSRC/api.hip -o $OUT/obj_$NAME/api.o &
wait
# every other object of the shipped build, whatever _build.py's HIP_SOURCES lists by now
REST=$(ls $OBJ/*.o | grep -v -e /lines_ms_kernel.o -e /api.o)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT/libmonortm_hip_$NAME.so $OUT/obj_$NAME/lines_ms_kernel.o $OUT/obj_$NAME/api.o $REST
ls -la $OUT/libmonortm_hip_$NAME.so
