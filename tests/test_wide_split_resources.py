"""Build-time guard (no GPU) on csrc/scan_wide.hip: no instantiation uses scratch memory -- the flagship form
scan_wide_kernel<384, 8, 24> holds its split list (12 slots per lane) AND the stagger's deferred accumulators inside the 256
registers a wave gets at two waves per SIMD -- and the ticket register of the 24- / 32-slot forms is untouched until its wait
(tools/check_resources.py).  One translation unit, ~1 minute."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wide_kernels_do_not_spill():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_resources.py"), "--list", "scan_wide.hip"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "0 violation(s)" in r.stdout
    m = re.search(r"scan_wide_kernel<384, 8, 24>\(.*?: (\d+) VGPRs, (\d+) B/lane of scratch", r.stdout)
    assert m, r.stdout[-3000:]
    assert int(m.group(1)) <= 256 and int(m.group(2)) == 0, m.group(0)
