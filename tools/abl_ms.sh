#!/bin/bash
# stage pricing of lines_ms_kernel on one box: tools/abl_ms.sh LIB "A1 A2 ..." [WORKLOAD] (LIB = an experiment build, MONORTM_MS_ABLATE values)
export OUT=${OUT:-bench_out}   # outputs of this script (per-kernel times come from bench.py --full)
mkdir -p $OUT/ab
export MONORTM_HIP_LIB=$PWD/$1
W=${3:-c4}
for r in 1 2; do for a in $2; do
  MONORTM_MS_ABLATE=$a python bench.py --full --workload $W --steps 100 --no-extra --no-cpu-baseline --no-pmc --detail-file $OUT/ab/d.json 2>$OUT/ab/err.txt >/dev/null || { tail -2 $OUT/ab/err.txt; continue; }
  python - $a $1 <<'P'
import os, json,sys
j=json.load(open(os.environ["OUT"] + "/ab/d.json")); print(f'{sys.argv[2]} ablate {sys.argv[1]} lines {j["kernel_ms_per_step"]["lines"]:.4f}')
P
done; done
