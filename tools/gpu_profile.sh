# One config's bench line + rocprofv3 kernel trace of a short run -> timed-step kernel stats and the
# per-stream timeline (busy time by kernel category, join analysis).
# usage: bash tools/gpu_profile.sh <tag> <model> [extra bench args]
set -o pipefail
export OUT=${OUT:-bench_out}   # where this script writes
TAG=$1; M=$2; shift 2
export TMPDIR=/tmp
mkdir -p $OUT
case $M in sdxl-lora|flux) SK=adamw_f32;; *) SK=adamw_bf16;; esac
timeout -k 10 400 python -u bench.py --model $M --no-cpu-baseline --no-vae "$@" > $OUT/bench_${TAG}_$M.json 2> $OUT/bench_${TAG}_$M.err || { echo "bench $M failed"; tail -30 $OUT/bench_${TAG}_$M.err; exit 1; }
cat $OUT/bench_${TAG}_$M.json
rm -rf $OUT/prof_${TAG}_$M
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG}_$M -o run -- python -u bench.py --full --model $M --steps 6 --warmup 2 --no-cpu-baseline --no-vae "$@" > $OUT/prof_${TAG}_$M.log 2>&1 || { echo "rocprof $M failed"; tail -30 $OUT/prof_${TAG}_$M.log; exit 1; }
DB=$(find $OUT/prof_${TAG}_$M -name '*.db' | head -1)
python tools/prof_summary.py "$DB" $OUT/kstats_${TAG}_$M.csv --steps-kernel $SK --top 40 > $OUT/kstats_${TAG}_$M.log 2>&1 || true
python tools/timeline.py "$DB" --marker $SK --top 25 > $OUT/timeline_${TAG}_$M.txt 2>&1 || true
rm -rf $OUT/prof_${TAG}_$M
head -20 $OUT/timeline_${TAG}_$M.txt
