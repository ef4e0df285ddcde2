# round-end rehearsal: full GPU suite, smoke(), the full bench line at the driver's step counts
# (python3 bench.py --gpus 1 --steps 20 --warmup 5 --full), and rocprofv3 kernel stats of a short bench
# outputs under $SM_OUT_DIR (default bench_out/)
set -e
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${SM_OUT_DIR:-bench_out}
mkdir -p $OUT
TAG=${1:-final}
timeout -k 10 900 python -u -m pytest -x -q --timeout 300 --timeout-method thread tests -m gpu > $OUT/${TAG}_gputests.log 2>&1
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/${TAG}_smoke.log 2>&1
timeout -k 10 500 python3 bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_prof -o run --output-format csv -- python bench.py --full --no-cpu-baseline --no-calibration --steps 3 --warmup 1 > $OUT/${TAG}_prof_bench.json 2> $OUT/${TAG}_prof_bench.err
python scripts/stepprof.py $OUT/${TAG}_prof --top 40 > $OUT/${TAG}_step_kernels.txt
