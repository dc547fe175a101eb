#!/bin/bash
# lines_ms_kernel against lines_kernel over batch sizes (rounds of waves) on one box: tools/rounds_sweep.sh "128 192 256 320 384 512 768" [WORKLOAD = c4shard, c2lc, c4brd]
export OUT=${OUT:-bench_out}   # outputs of this script (per-kernel times come from bench.py --full)
mkdir -p $OUT/ab
for n in $1; do for k in wn ms auto; do
  MONORTM_LINES_KERNEL=$k python bench.py --full --workload ${2:-c4shard} --profiles-per-gpu $n --steps 100 --no-extra --no-cpu-baseline --no-pmc --detail-file $OUT/ab/d.json 2>$OUT/ab/err.txt >/dev/null || { tail -2 $OUT/ab/err.txt | cut -c1-200; continue; }
  python - $n $k <<'P'
import os, json,sys
j=json.load(open(os.environ["OUT"] + "/ab/d.json")); print(f'{sys.argv[1]:>5s} profiles {sys.argv[2]:4s} lines {j["kernel_ms_per_step"]["lines"]:.4f} step {j["ms_per_step"]:.4f}')
P
done; done
