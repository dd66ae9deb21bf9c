#!/bin/bash
# Round-4 artifacts for profiles/ (GPU box, repo root): scripts/collect_profiles_r04.sh <commit>
#   PMC traffic of the bench command (two passes) -> r04_pmc_ingest_kernels.json / r04_pmc_summary.txt   (first: bench.py quotes it)
#   the bench line at the driver's flags                       -> r04_bench_final.json
#   rocprofv3 --kernel-trace --stats of the same command       -> r04_bench_final_kernel_stats.csv
#   bsc_ingest alone (sync per call) under rocprofv3            -> r04_ingest_isolated_kernel_stats.csv
#   the f32 encoder (split-operand GEMMs, piece attention) alone -> r04_encoder_f32_kernel_stats.csv
#   SQ MFMA counters of the f32 encoder's and the bf16 encoder's kernels -> r04_pmc_mfma_counters.txt
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${OUT:-$ROOT/out}"                 # where the outputs go
commit=${1:-unknown}
export TMPDIR=/tmp
mkdir -p $OUT
bash scripts/pmc_ingest.sh r04 $commit > /dev/null
cp $OUT/r04_pmc_ingest_kernels.json profiles/r04_pmc_ingest_kernels.json
cp $OUT/r04_pmc_summary.txt profiles/r04_pmc_summary.txt
timeout 900 python bench.py --full --steps 20 --warmup 5 > $OUT/r04_bench_final.json 2> $OUT/r04_bench_final.err
rm -rf /tmp/prof_stats
( cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_stats -- python $ROOT/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-workloads --no-localize --no-exact --no-f32 > $OUT/r04_bench_under_rocprof.json 2>/dev/null )
cp $(find /tmp/prof_stats -name "*kernel_stats.csv" | head -1) $OUT/r04_bench_final_kernel_stats.csv
LINES_MAX=1 bash scripts/prof_iso.sh $OUT/r04_ingest_isolated_kernel_stats.csv 6 sync 384 room > /dev/null
rm -rf /tmp/pf32
( cd /tmp && timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/pf32 -- python $ROOT/scripts/encoder_f32_only.py vit_b16 384 1 > $OUT/r04_encoder_f32.log 2>&1 )
cp $(find /tmp/pf32 -name "*kernel_stats.csv" | head -1) $OUT/r04_encoder_f32_kernel_stats.csv
rm -rf /tmp/pmc_mfma
( cd /tmp && timeout 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU_MFMA_MOPS_F16 SQ_INSTS_VALU_MFMA_MOPS_BF16 SQ_WAVE_CYCLES SQ_WAVES GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d /tmp/pmc_mfma -- python $ROOT/scripts/encoder_f32_only.py vit_b16 384 1 > /dev/null 2>&1 )
python scripts/pmc_generic.py $(find /tmp/pmc_mfma -name "*counter_collection.csv" | head -1) "k_" > $OUT/r04_pmc_mfma_counters.txt
rm -rf /tmp/pmc_mfma2
( cd /tmp && timeout 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU_MFMA_MOPS_F16 SQ_INSTS_VALU_MFMA_MOPS_BF16 SQ_WAVE_CYCLES SQ_WAVES GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d /tmp/pmc_mfma2 -- python $ROOT/scripts/encoder_only.py vit_b16 384 > /dev/null 2>&1 )
python scripts/pmc_generic.py $(find /tmp/pmc_mfma2 -name "*counter_collection.csv" | head -1) "" | grep -E "Cijk|k_attention|k_bias|k_embed|k_preprocess" >> $OUT/r04_pmc_mfma_counters.txt
ls -la $OUT/r04_*
