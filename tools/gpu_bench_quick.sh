# the bench line without the CPU leg, then rocprof kernel stats of the eager step
# usage: bash tools/gpu_bench_quick.sh [output directory, default build/evidence]
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-$R/build/evidence}
mkdir -p $OUT
cd $R
python bench.py --steps 10 --warmup 3 --full --no-cpu-baseline > $OUT/b_graph.log 2>&1; echo rc=$?
grep -v amdgpu.ids $OUT/b_graph.log | tail -5
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_eager -- python3 $R/bench.py --steps 3 --warmup 2 --full --no-graph --no-cpu-baseline > $OUT/prof_eager.log 2>&1; echo rc=$?
cd $R
ls -R $OUT/prof_eager | head -20
