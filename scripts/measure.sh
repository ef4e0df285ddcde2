# Measurement set: full bench line (bench.py --full), rocprofv3 kernel stats of the same command,
# per-op ledger, PMC HBM traffic of the roofline kernels (separate FETCH/WRITE passes).
# usage: bash scripts/measure.sh TAG      (outputs under $SM_OUT_DIR, default bench_out/)
set -e
TAG=${1:-r02}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${SM_OUT_DIR:-bench_out}
mkdir -p $OUT
timeout -k 10 400 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_prof -o run --output-format csv -- python bench.py --full --no-cpu-baseline --steps 3 --warmup 1 > $OUT/${TAG}_prof_bench.json 2> $OUT/${TAG}_prof_bench.err
timeout -k 10 300 python scripts/ledger.py --top 80 > $OUT/${TAG}_ledger.txt 2> $OUT/${TAG}_ledger.err
timeout -s KILL 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/${TAG}_pmc_fetch -o run --output-format csv -- python bench.py --steps 1 --warmup 1 > $OUT/${TAG}_pmc_fetch.log 2>&1
timeout -s KILL 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/${TAG}_pmc_write -o run --output-format csv -- python bench.py --steps 1 --warmup 1 > $OUT/${TAG}_pmc_write.log 2>&1
timeout -k 10 120 python scripts/pmc_traffic.py $OUT/${TAG}_pmc_fetch $OUT/${TAG}_pmc_write "attn_bwd_dq_bf16<64, true>+attn_bwd_dkdv_bf16<64, true>" $OUT/${TAG}_traffic.json
timeout -k 10 120 python scripts/pmc_traffic.py $OUT/${TAG}_pmc_fetch $OUT/${TAG}_pmc_write "attn_fwd_bf16<64, true>" $OUT/${TAG}_traffic_fwd.json
timeout -k 10 120 python scripts/pmc_table.py $OUT/${TAG}_pmc_fetch $OUT/${TAG}_pmc_write 80 > $OUT/${TAG}_traffic_table.txt
