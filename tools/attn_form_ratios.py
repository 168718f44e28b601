#!/usr/bin/env python3
"""profiles/attn_forms_ratios.txt from the output of the attention form tests (needs that output, no GPU):

  python -m pytest -q -s -m gpu tests/test_attn_forms_gpu.py > run.log
  python tools/attn_form_ratios.py run.log > profiles/attn_forms_ratios.txt

Every case prints "attn-ratio <max |err| / bound> <case id> | <kernel with template arguments>"; this keeps the largest ratio per
instantiation, the case it came from and the smallest one, and the "attn-bit-equal" lines of the whole-sequence kernel against the
blocked one.  The numbers are observations: the tests assert the derived bound of tests/_attn_ref.py alone (ratio <= 1)."""
import sys

best, low, count, equal = {}, {}, {}, {}
for line in open(sys.argv[1]):
    if "attn-bit-equal" in line:
        f = line[line.index("attn-bit-equal") + len("attn-bit-equal"):].split(" vs ")
        key = f[0].strip()
        equal.setdefault(key, []).append(": True" in f[1])
        continue
    if "attn-ratio" not in line:
        continue
    f = line[line.index("attn-ratio"):].split(None, 2)      # (the line may begin with pytest's progress dots)
    ratio, (case, kernel) = float(f[1]), [s.strip() for s in f[2].split("|")]
    count[kernel] = count.get(kernel, 0) + 1
    low[kernel] = min(low.get(kernel, ratio), ratio)
    if kernel not in best or ratio > best[kernel][0]:
        best[kernel] = (ratio, case)
print("# largest (and smallest) max|err| / bound per attention kernel instantiation (tests/test_attn_forms_gpu.py; MI355X)")
print(f"# {'kernel':40s} {'cases':>5s} {'max':>7s} {'min':>7s}  case of the maximum")
for kernel, (ratio, case) in sorted(best.items()):
    print(f"{kernel:42s} {count[kernel]:5d} {ratio:7.4f} {low[kernel]:7.4f}  {case}")
for kernel, flags in sorted(equal.items()):
    print(f"# {kernel}: bit-equal to the blocked kernel in {sum(flags)} of {len(flags)} cases")
