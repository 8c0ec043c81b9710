# Bench line + timed-step rocprof kernel stats for BASELINE configs.  usage: bash tools/gpu_configs.sh <tag> <model>...
# (model: sdxl | sd15 | sdxl-lora | flux; the optimizer kernel that marks step boundaries is picked per model)
set -o pipefail
export OUT=${OUT:-bench_out}   # where this script writes
TAG=$1; shift
export TMPDIR=/tmp
mkdir -p $OUT
for M in "$@"; do
  case $M in sdxl-lora|flux) SK=adamw_f32;; *) SK=adamw_bf16;; esac
  timeout -k 10 500 python -u bench.py --model $M --no-cpu-baseline --no-vae > $OUT/bench_${TAG}_$M.json 2> $OUT/bench_${TAG}_$M.err || { echo "bench $M failed"; tail -30 $OUT/bench_${TAG}_$M.err; exit 1; }
  cat $OUT/bench_${TAG}_$M.json
  rm -rf $OUT/prof_${TAG}_$M
  timeout -k 10 500 rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG}_$M -o run -- python -u bench.py --full --model $M --steps 6 --warmup 2 --no-cpu-baseline --no-vae > $OUT/prof_${TAG}_$M.log 2>&1 || { echo "rocprof $M failed"; tail -30 $OUT/prof_${TAG}_$M.log; exit 1; }
  DB=$(find $OUT/prof_${TAG}_$M -name '*.db' | head -1)
  python tools/prof_summary.py "$DB" $OUT/kstats_${TAG}_$M.csv --steps-kernel $SK --top 30 > $OUT/kstats_${TAG}_$M.log 2>&1 || true
  find $OUT/prof_${TAG}_$M -name '*kernel_stats.csv' -exec cp {} $OUT/rocprof_stats_${TAG}_$M.csv \; || true
  rm -rf $OUT/prof_${TAG}_$M
  head -12 $OUT/kstats_${TAG}_$M.log
done
