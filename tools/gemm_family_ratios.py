#!/usr/bin/env python3
"""profiles/gemm_families_ratios.txt from the output of the GEMM family tests (needs that output, no GPU):

  python -m pytest -q -s -m gpu tests/test_gemm_families_gpu.py tests/test_proj_ln_gpu.py > run.log
  python tools/gemm_family_ratios.py run.log > profiles/gemm_families_ratios.txt

Every case prints "gemm-ratio <family> mode <m> <max |err| / bound> <case id> setting <index>" (the children's lines come through their
parent); this keeps the largest ratio per family and mode, and the case it came from.  The numbers are observations: the tests assert
the derived bound of tests/_gemm_ref.py alone (ratio <= 1)."""
import sys

best, count = {}, {}
for line in open(sys.argv[1]):
    if "gemm-ratio" not in line:
        continue
    f = line[line.index("gemm-ratio"):].split()      # (the line may begin with pytest's progress dots)
    key, ratio, case = (f[1], f[3]), float(f[4]), f"{f[5]} (setting {f[7]})"
    count[key] = count.get(key, 0) + 1
    if key not in best or ratio > best[key][0]:
        best[key] = (ratio, case)
print("# largest max|err| / bound per kernel family and mode (tests/test_gemm_families_gpu.py, tests/test_proj_ln_gpu.py; MI355X)")
print(f"# {'family':32s} {'mode':>4s} {'cases':>5s} {'ratio':>7s}  case")
for (family, mode), (ratio, case) in sorted(best.items()):
    print(f"{family:34s} {mode:>4s} {count[(family, mode)]:5d} {ratio:7.4f}  {case}")
