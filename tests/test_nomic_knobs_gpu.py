"""GPU: GEMM mode 4 (the gated epilogue) on its own under every knob setting that changes which kernel serves it or which of its
instantiations runs.  The knobs are read once per process, so every setting but the default runs in one fresh child process (pytest
on this file), one at a time, as tests/test_gemm_families_gpu.py does.  Every case asserts the kernel WITH ITS TEMPLATE ARGUMENTS
from crs_gemm_plan_describe before it launches (on a device whose CU count is not the table's 256 a case whose line differs skips
and says so; on an MI355X nothing skips), then holds every element to tests/_gated_ref.py's derived bound, with and without a bias,
on an output framed by canary rows.

What the settings move (csrc/enc_plan.cpp: plan_gemm with mode 4 answers gemm8 where gemm8_applies, else the tiled kernel):
  CRS_GEMM8_MIN_WGS=1            the 256 x 256 kernel takes over from the tiled kernel at small shapes: one tile, half a last column
                                 block, several tiles (tests/_gemm_cases.py: G8_SMALL, n = 2F here), one workgroup per item
  ... + CRS_GEMM8_VAR=1 / 2 / 3  its schedule variants gemm8_kernel<4, false, 1..3>; with 264 items (more than the CUs) variants 2
                                 and 3 also run their persistent forms <4, true, 2 | 3> (variant 1 has none: one workgroup per item)
  CRS_GEMM8=0                    the index-build shapes leave gemm8 for the tiled kernel (mode 4 never takes the 256-row or the
                                 row-streaming kernels, whatever CRS_GEMM_BIG* / CRS_GEMM_STREAM say: two more settings hold that)
The index-build shape 32768 x 6144 x 768 itself is left out: its fp64 reference is 3e11 operations on the CPU; 2816 x 3072 x 384 / 768
and 16384 x 384 x 384 are the smallest row counts gemm8 accepts at those widths and run the same code."""
import os
import re
import subprocess
import sys
from collections import namedtuple

import pytest

import _gated_ref as gt
import _gemm_ref as gr

pytestmark = pytest.mark.gpu

TABLE_CUS = 256
SETTINGS = [
    {},
    {"CRS_GEMM8_MIN_WGS": "1"},
    {"CRS_GEMM8_MIN_WGS": "1", "CRS_GEMM8_VAR": "1"},
    {"CRS_GEMM8_MIN_WGS": "1", "CRS_GEMM8_VAR": "2"},
    {"CRS_GEMM8_MIN_WGS": "1", "CRS_GEMM8_VAR": "3"},
    {"CRS_GEMM8": "0"},
    {"CRS_GEMM8": "0", "CRS_GEMM_BIG_MIN_WGS": "1"},                       # modes 0 / 1 would take the 256-row kernel here
    {"CRS_GEMM_STREAM": "0", "CRS_GEMM8": "0", "CRS_GEMM_BIG": "0"},       # everything on the tiled kernel, as the A/B settings run it
]
Case = namedtuple("Case", "setting m f k kernel")
G8_SMALL = [(256, 128, 256), (256, 192, 384), (512, 320, 896)]             # (m, F, k): n = 2F = 256, 384, 640
G8_INDEX = [(2816, 1536, 384), (2816, 1536, 768), (16384, 192, 384)]       # the smallest row counts gemm8 accepts by default
PERSIST = (5632, 1536, 384)                                                # 22 x 12 = 264 items > 256 CUs
CASES = [Case(0, 257, 256, 512, "gemm_f16_kernel<4>")]                     # (default: modes 0 / 1 of this shape are not tiled)
for si, var in [(1, 0), (2, 1), (3, 2), (4, 3)]:
    CASES += [Case(si, m, f, k, f"gemm8_kernel<4, false, {var}>") for m, f, k in G8_SMALL]
    if var:
        CASES.append(Case(si, *PERSIST, f"gemm8_kernel<4, {'false' if var == 1 else 'true'}, {var}>"))
for si in (5, 7):
    CASES += [Case(si, m, f, k, "gemm_f16_kernel<4>") for m, f, k in G8_INDEX]
CASES += [Case(6, m, f, k, "gemm_f16_kernel<4>") for m, f, k in [(257, 128, 512), (511, 384, 640), G8_INDEX[0]]]

CHILD_ENV = "NOMIC_KNOBS_SETTING"
SI = int(os.environ.get(CHILD_ENV, "0"))
HERE = [c for c in CASES if c.setting == SI]
_failed = []


def _id(c):
    return f"s{c.setting}-{c.m}x{2 * c.f}x{c.k}"


@pytest.mark.parametrize("c", HERE, ids=[_id(c) for c in HERE])
def test_gated_case(cuda, c):
    import torch
    from rag._encoder import gemm_f16_routed, gemm_plan_describe
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    line, slabs = gemm_plan_describe(c.m, 2 * c.f, c.k, 4, 0, 0)
    kernel = line.split(" grid=")[0]
    if kernel != c.kernel and cus != TABLE_CUS:
        pytest.skip(f"the case table was written for {TABLE_CUS} CUs; this device has {cus} and plans {kernel}, not {c.kernel}")
    assert kernel == c.kernel and slabs == 1, line
    a, w, bias = gt.make_inputs(c.m, c.f, c.k)
    ps = gr.products(a, w, 1)
    frame = 8
    for b in (bias, None):
        ref, bound = gt.gated_ref_and_bound(a, w, b, ps=ps)
        out = torch.full((c.m + 2 * frame, c.f), 7.0, dtype=torch.float16, device=cuda)
        out[frame:-frame] = float("nan")                       # an element the kernel does not write fails as well
        gemm_f16_routed(a.to(cuda), w.to(cuda), None if b is None else b.to(cuda), None, out[frame:frame + c.m], 4, 0, 0)
        torch.cuda.synchronize()
        got = out.cpu()
        assert (got[:frame] == 7.0).all() and (got[-frame:] == 7.0).all()
        assert not torch.isnan(got).any()
        r = gr.ratio(got[frame:-frame], ref, bound)
        print("gated-ratio", kernel, _id(c), "bias" if b is not None else "no bias", r)
        assert r <= 1.0


@pytest.mark.skipif(SI != 0, reason="the parent process starts the children")
@pytest.mark.parametrize("si", range(1, len(SETTINGS)), ids=["+".join(f"{k}={v}" for k, v in s.items()) for s in SETTINGS[1:]])
def test_setting_in_child_process(cuda, si):
    if _failed:
        pytest.fail(f"not started: the child of setting {SETTINGS[_failed[0]]} failed")
    n = sum(c.setting == si for c in CASES)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **SETTINGS[si])
    env[CHILD_ENV] = str(si)
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__),
                            "-k", "test_gated_case"], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _failed.append(si)
        raise
    print("".join(line[line.index("gated-ratio"):] + "\n" for line in r.stdout.splitlines() if "gated-ratio" in line), end="")
    if r.returncode != 0:
        _failed.append(si)
    assert r.returncode == 0, str(SETTINGS[si]) + r.stdout[-3000:] + r.stderr[-2000:]
    tail = r.stdout.strip().splitlines()[-1]
    passed = int((re.search(r"(\d+) passed", tail) or [0, 0])[1])
    skipped = int((re.search(r"(\d+) skipped", tail) or [0, 0])[1])
    assert passed + skipped == n, (SETTINGS[si], tail)          # the child ran exactly this setting's cases
    if skipped:
        pytest.skip(f"{skipped} of {n} cases skipped in the child: the case table was written for {TABLE_CUS} CUs")
