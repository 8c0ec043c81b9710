# Round 6: C4 timed-step kernel trace at HEAD (kernel stats + stream timeline)
set -o pipefail
export OUT=${OUT:-bench_out}   # where this script writes
export TMPDIR=/tmp; mkdir -p $OUT
P=$OUT/prof_r6k; rm -rf $P
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $P -o run -- python3 -u bench.py --full --model sdxl-lora --steps 8 --warmup 2 --no-cpu-baseline --no-vae > $P.log 2>&1 || { tail -30 $P.log; exit 1; }
DB=$(find $P -name '*.db' | head -1)
python3 tools/prof_summary.py "$DB" $OUT/r6k_kstats_sdxl-lora.csv --steps-kernel adamw_f32 --top 40 > $OUT/r6k_kstats_sdxl-lora.log 2>&1; head -5 $OUT/r6k_kstats_sdxl-lora.log
python3 tools/timeline.py "$DB" --marker adamw_f32 > $OUT/r6k_timeline_sdxl-lora.txt 2>&1; head -48 $OUT/r6k_timeline_sdxl-lora.txt
rm -rf $P $P.log
