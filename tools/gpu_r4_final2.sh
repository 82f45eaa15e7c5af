#!/bin/bash
OUT=${1:?usage: tools/gpu_r4_final2.sh OUTDIR}
mkdir -p $OUT
bash tools/profile_r4.sh r04b stats > $OUT/final_profile_stats.log 2>&1
timeout 900 python bench.py --full > $OUT/final_bench_default.log 2>$OUT/final_bench_default.err
