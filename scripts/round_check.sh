# full GPU test suite + full bench line (bench.py --full: calibration, roofline probes, CPU baselines)
# outputs under $SM_OUT_DIR (default bench_out/)
set -e
TAG=${1:-r02x}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${SM_OUT_DIR:-bench_out}
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest -x -q --timeout 300 --timeout-method thread tests -m gpu > $OUT/${TAG}_gputests.log 2>&1
timeout -k 10 400 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
