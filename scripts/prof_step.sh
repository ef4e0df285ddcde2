# full bench line (bench.py --full) + rocprofv3 kernel stats of the same command + per-step category summary
# outputs under $SM_OUT_DIR (default bench_out/)
set -e
TAG=${1:-r02x}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${SM_OUT_DIR:-bench_out}
mkdir -p $OUT
timeout -k 10 400 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_prof -o run --output-format csv -- python bench.py --full --no-cpu-baseline --steps 3 --warmup 1 > $OUT/${TAG}_prof_bench.json 2> $OUT/${TAG}_prof_bench.err
python scripts/stepprof.py $OUT/${TAG}_prof --top 40 > $OUT/${TAG}_summary.txt
