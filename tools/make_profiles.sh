#!/bin/bash
# Collect the round's evidence on one GPU machine: --full bench lines for every workload, the
# rocprofv3 kernel-trace stats of the same commands, and separate --pmc passes (FETCH_SIZE, WRITE_SIZE)
# for the default workload.  Outputs land in $OUT/<TAG>_* (default profile_runs/); tools/pmc_summary.py turns them into
# profiles/.   usage: tools/make_profiles.sh TAG [workloads...]
set -o pipefail
TAG=${1:-r02}; shift
WL=${@:-c4 c5 c3 c2}
cd "$(dirname "$0")/.."
export OUT=${OUT:-profile_runs}
mkdir -p $OUT
for w in $WL; do
  extra="--full"; [ $w != c4 ] && extra="--full --no-cpu-baseline"
  python3 bench.py --workload $w $extra > $OUT/${TAG}_bench_$w.json 2> $OUT/${TAG}_bench_$w.err || { tail -5 $OUT/${TAG}_bench_$w.err; exit 1; }
  echo "bench $w done: $(cut -c1-200 $OUT/${TAG}_bench_$w.json)"
  # kernel-trace stats of the same command; program directly after --
  rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_stats_$w -- python3 bench.py --workload $w --full --no-cpu-baseline > $OUT/${TAG}_stats_$w.log 2>&1 || { tail -5 $OUT/${TAG}_stats_$w.log; exit 1; }
  echo "stats $w done"
done
# encoder index-build workloads (bench line + kernel stats of the same command)
for w in enc-minilm enc-bge; do
  python3 bench.py --workload $w --steps 20 --warmup 3 > $OUT/${TAG}_bench_$w.json 2> $OUT/${TAG}_bench_$w.err || { tail -5 $OUT/${TAG}_bench_$w.err; exit 1; }
  echo "bench $w done: $(cut -c100-240 $OUT/${TAG}_bench_$w.json)"
  rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_stats_$w -- python3 bench.py --workload $w --steps 20 --warmup 3 > $OUT/${TAG}_stats_$w.log 2>&1 || { tail -5 $OUT/${TAG}_stats_$w.log; exit 1; }
  echo "stats $w done"
done
# PMC passes: counters only with --kernel-trace (one --pmc set per run)
for w in c4; do
  for c in FETCH_SIZE WRITE_SIZE; do
    rocprofv3 --pmc $c --kernel-trace --output-format csv -d $OUT/${TAG}_pmc_${c}_$w -- python3 bench.py --workload $w --steps 6 --warmup 1 --streams 1 --no-graph --full --no-cpu-baseline > $OUT/${TAG}_pmc_${c}_$w.log 2>&1 || { tail -5 $OUT/${TAG}_pmc_${c}_$w.log; exit 1; }
  done
  echo "pmc $w done"
done
