# MFMA utilisation of one SDXL train step from PMC counters (one pass: 2 SQ + 1 GRBM counters, kernel
# trace only).  usage: bash tools/gpu_mfma.sh <tag> [bench args...]
set -o pipefail
export OUT=${OUT:-bench_out}   # where this script writes
TAG=${1:-mfma}
shift || true
export TMPDIR=/tmp
mkdir -p $OUT
rm -rf $OUT/pmc_${TAG}
timeout -s KILL 240 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES GRBM_GUI_ACTIVE --kernel-trace --output-format csv \
  -d $OUT/pmc_${TAG} -o run -- python3 -u bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-vae "$@" \
  > $OUT/pmc_${TAG}.log 2>&1 || { echo "mfma pass failed"; tail -20 $OUT/pmc_${TAG}.log; exit 1; }
python3 tools/pmc_mfma.py $OUT/pmc_${TAG} $OUT/pmc_${TAG}.json > /dev/null && rm -rf $OUT/pmc_${TAG} && head -c 3000 $OUT/pmc_${TAG}.json
