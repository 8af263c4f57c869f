# end-of-round evidence: bench line, rocprof kernel stats of the same command, calibrated PMC traffic of the hot kernels
# usage: bash tools/gpu_round_artifacts.sh [output directory, default build/evidence]
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-$R/build/evidence}
mkdir -p $OUT
cd $R
python bench.py --steps 20 --warmup 5 --full > $OUT/bench_full.log 2>&1; echo bench rc=$?
grep -v "amdgpu.ids\|Warning\|run_backward" $OUT/bench_full.log | tail -1 > $OUT/bench_line.json; cat $OUT/bench_line.json | cut -c1-200
cd /tmp && export TMPDIR=/tmp
rm -rf /tmp/prof_bench /tmp/pmc_k /tmp/pmc_c
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_bench -- python3 $R/bench.py --steps 5 --warmup 2 --full --no-cpu-baseline > $OUT/prof_bench.log 2>&1; echo prof rc=$?
f=$(ls /tmp/prof_bench/*/*kernel_stats.csv | head -1)
head -1 $f > $OUT/bench_kernel_stats_td.csv; grep -E "(^\"|[^s])td::" $f >> $OUT/bench_kernel_stats_td.csv
for pass in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --pmc $pass --output-format csv -d /tmp/pmc_k/$pass -- python3 $R/tools/kernel_bench.py --iters 3 --only identity,fwd,bwd > $OUT/pmc_$pass.log 2>&1; echo "$pass rc=$?"
  rocprofv3 --pmc $pass --output-format csv -d /tmp/pmc_c/$pass -- python3 $R/tools/kernel_bench.py --iters 3 --only calib > $OUT/pmc_calib_$pass.log 2>&1; echo "calib $pass rc=$?"
done
cd $R
python tools/traffic_from_pmc.py /tmp/pmc_k /tmp/pmc_c > $OUT/traffic.json 2> $OUT/traffic.err; cat $OUT/traffic.json; tail -3 $OUT/traffic.err
python tools/pmc_summary.py /tmp/pmc_k > $OUT/pmc_summary.txt 2>&1
cat $OUT/bench_kernel_stats_td.csv | cut -c1-200
