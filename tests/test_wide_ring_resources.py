"""Build-time guard (no GPU) on csrc/scan_wide_ring.hip, the ring kernels of csrc/scan_wide.hip ("Ring form"):

  * tools/check_resources.py finds no violation; ring::scan_wide16_kernel<384, 8, 24> is the only kernel of the file, stays within the
    256 registers a wave has at two waves per SIMD and uses no scratch;
  * the loop in the device assembly is the one the header describes: behind the prologue's barrier the kernel holds exactly one
    s_barrier (the loop's) and four s_waitcnt with a vmcnt -- one per issue site (idle waves, waves 0-3, waves 4-7) and the guard
    behind the loop -- all of them vmcnt(0) written in the source: the compiler adds none, so nothing drains a transfer inside the MFMA
    sweep or between a wave's issue and the barrier.  Behind each of the loop's three waits the next memory or matrix instruction is a
    global_load_lds (wait, then issue), and the barrier is preceded by an lgkmcnt(0) alone;
  * the ticket: the register the asm global_atomic_add returns into is named by no instruction between the atomic and the wait of
    waves 0-3 (the second vmcnt(0) behind the atomic: the first is the idle waves', whose path never reads it), and the first
    instruction that does name it lies behind that wait.
~1 minute."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "compressed-rag-suite_amd", "csrc", "scan_wide_ring.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_ring_kernel_fits_its_registers():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_resources.py"), "--list", "scan_wide_ring.hip"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "0 violation(s)" in r.stdout
    rows = re.findall(r"kernel\s+scan_wide_ring.hip: .*?::(ring::\w+)<(\d+), (\d+), (\d+)>\(.*?: (\d+) VGPRs, (\d+) B/lane of scratch", r.stdout)
    assert len(rows) == r.stdout.count("  kernel ")
    assert [(n, int(d), int(nw), int(k)) for n, d, nw, k, _, _ in rows] == [("ring::scan_wide16_kernel", 384, 8, 24)], r.stdout[-2000:]
    assert int(rows[0][4]) <= 256 and int(rows[0][5]) == 0, rows


def _mentions(line, reg):
    code = line.split(";")[0]
    if any(int(x) == reg for x in re.findall(r"\bv(\d+)\b", code)):
        return True
    return any(int(a) <= reg <= int(b) for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", code))


def test_ring_loop_in_the_device_assembly():
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", SRC, "-o", "-"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"^(_Z\S*4ring18scan_wide16_kernelILi384ELi8ELi24E\S*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", r.stdout, flags=re.S | re.M)
    assert len(kernels) == 1
    lines = [ln.strip() for ln in kernels[0][1].splitlines() if ln.strip() and not ln.lstrip().startswith(";")]
    barriers = [i for i, ln in enumerate(lines) if ln.startswith("s_barrier")]
    assert len(barriers) == 2, barriers                     # the prologue's and the loop's
    loop = lines[barriers[0] + 1:]
    waits = [i for i, ln in enumerate(loop) if ln.startswith("s_waitcnt") and "vmcnt" in ln]
    assert [loop[i] for i in waits] == ["s_waitcnt vmcnt(0)"] * 4, [loop[i] for i in waits]
    bar = barriers[1] - barriers[0] - 1
    assert waits[2] < bar < waits[3]                        # three in the loop, the guard behind it
    assert loop[bar - 1] == "s_waitcnt lgkmcnt(0)", loop[bar - 3:bar + 1]
    heavy = re.compile(r"(global_|ds_read|ds_write|v_mfma|s_barrier|buffer_|scratch_|flat_)")
    for w in waits[:3]:
        nxt = next(ln for ln in loop[w + 1:] if heavy.match(ln))
        assert nxt.startswith("global_load_lds_dwordx4"), (w, nxt)
    assert sum(ln.startswith("v_mfma_f32_16x16x32_f16") for ln in loop[:bar]) == 2 * 96      # one sweep per wave half, no more
    draws = [i for i, ln in enumerate(loop) if ln.startswith("global_atomic_add")]
    assert len(draws) == 1 and draws[0] < waits[0]
    reg = int(re.match(r"global_atomic_add\s+v(\d+),", loop[draws[0]]).group(1))
    first_use = next(i for i in range(draws[0] + 1, len(loop)) if _mentions(loop[i], reg))
    assert waits[1] < first_use < waits[2], (reg, loop[first_use], waits)
