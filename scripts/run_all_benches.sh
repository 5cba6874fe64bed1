#!/bin/bash
# Run on the GPU box (through gpurun): one bench.py line per workload into gpurun_out/<tag>_<WL>.json
# usage: scripts/run_all_benches.sh <tag> [workloads...]
# (the engines outside bench.py have their own scripts, one JSON line per measurement:
#  bench_spiral.py, bench_hees.py, bench_nshs.py, bench_lm.py, bench_xnes.py, bench_amalgam.py,
#  bench_slpso.py, bench_crs.py, bench_ssde.py, bench_mayfly.py, bench_pikaia.py, bench_neldermead.py, bench_rosenbrock.py,
#  bench_basinhopping.py,
#  bench_program_objective.py)
TAG=$1; shift
WLS=${@:-"M C1 C3 C2 JADE SANSDE SEP CSO CCPSO C4 C5"}
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
mkdir -p $ROOT/gpurun_out
for WL in $WLS; do
  STEPS=100; [ "$WL" = "C4" ] && STEPS=20; [ "$WL" = "C5" ] && STEPS=2
  timeout -k 10 400 python3 $ROOT/bench.py --workload $WL --steps $STEPS --warmup 10 --full \
      > $ROOT/gpurun_out/${TAG}_$WL.json 2> $ROOT/gpurun_out/${TAG}_$WL.err
  echo "$WL rc=$? $(head -c 180 $ROOT/gpurun_out/${TAG}_$WL.json)"
done
