"""Build-time guard (no GPU) on csrc/scan_wide.hip with the deferred insertion (pending slot + bound: three more registers per
lane in the forms of wide_defer<>): tools/check_resources.py finds no violation in the file, every split-list kernel (24 / 32
slots) of both MFMA shapes is free of scratch, and <384, 8, 24> of both shapes stays within the 256 registers a wave has at two
waves per SIMD.  ~20 s."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split_list_kernels_keep_their_registers():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_resources.py"), "--list", "scan_wide.hip"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "0 violation(s)" in r.stdout
    rows = {(name, int(d), int(nw), int(k)): (int(v), int(s)) for name, d, nw, k, v, s in
            re.findall(r"(scan_wide(?:16)?_kernel)<(\d+), (\d+), (\d+)>\(.*?: (\d+) VGPRs, (\d+) B/lane of scratch", r.stdout)}
    split = {key: val for key, val in rows.items() if key[3] in (24, 32)}
    want = {("scan_wide_kernel", d, nw, k) for d in (128, 256, 384) for nw in (4, 8) for k in (24, 32)}
    want |= {("scan_wide16_kernel", d, 8, k) for d in (256, 384) for k in (24, 32)}
    assert set(split) == want, sorted(set(split) ^ want)
    assert all(s == 0 for _, s in split.values()), {key: val for key, val in split.items() if val[1]}
    for name in ("scan_wide_kernel", "scan_wide16_kernel"):
        assert split[(name, 384, 8, 24)][0] <= 256, (name, split[(name, 384, 8, 24)])
