#!/bin/bash
# Scan-only sweep over query-batch sizes (diagnostic): tools/sweep_q.sh "c3 c2 c4" "256 512"
WL=${1:-"c3 c2 c4"}; QS=${2:-"256 512"}
for w in $WL; do for q in $QS; do
  python bench.py --workload $w --queries $q --scan-only --full --no-cpu-baseline --steps 50 --warmup 5 2>/dev/null | python -c "
import json, sys
d = json.loads(sys.stdin.read().strip().splitlines()[-1])
print('$w', $q, 'q/s', d['value'], 'ms/step', d['ms_per_step'], 'scan_ms', d['roofline']['kernel_ms'], 'frac', d['roofline']['frac'], 'check_ok', d['config']['check_ok'])" || exit 1
done; done
