"""The cases of tests/test_gemm_families_gpu.py and tests/test_proj_ln_gpu.py: every encoder GEMM kernel family on its own, at the
smallest shapes at which each of its mechanisms can still go wrong.  A case names its knob setting (an index into SETTINGS; the knobs
are read once per process, so every setting but {} runs in a fresh child), the planner route, the shape, the mode and the KERNEL WITH
TEMPLATE ARGUMENTS IT MUST RUN, as the planner picks it on a 256-CU device (MI355X).  tests/test_gemm_ref_cpu.py holds this table to
the planner without a device; the GPU tests assert it from crs_gemm_plan_describe / crs_proj_ln_plan_describe before they launch."""
import os
import re
import subprocess
import sys
from collections import namedtuple

TABLE_CUS = 256

SETTINGS = [
    {},
    {"CRS_PANEL_KC": "128"},                                  # 1: the panel kernel stages 128 columns at a time everywhere
    {"CRS_PANEL_KC": "256"},                                  # 2: ... keeps its one-shot chunk beyond one wave of workgroups
    {"CRS_PANEL_MAX_SPLIT": "8"},                             # 3: up to 8 slabs
    {"CRS_GEMM8_MIN_WGS": "1"},                               # 4: the 256 x 256 kernel from one tile on, one workgroup per item
    {"CRS_GEMM8_MIN_WGS": "1", "CRS_GEMM8_VAR": "1"},         # 5..7: its schedule variants
    {"CRS_GEMM8_MIN_WGS": "1", "CRS_GEMM8_VAR": "2"},
    {"CRS_GEMM8_MIN_WGS": "1", "CRS_GEMM8_VAR": "3"},
    {"CRS_GEMM8": "0", "CRS_GEMM_BIG_MIN_WGS": "1"},          # 8: the 256-row pipelined kernel from one workgroup on
    {"CRS_GEMM_STREAM": "0", "CRS_GEMM8": "0", "CRS_GEMM_BIG": "0"},   # 9: everything on the tiled kernel, as the A/B settings run it
    {"CRS_ROWLN2_VARIANT": "0"},                              # 10: the fused projection + LayerNorm's <32, 4> ring
]

# route 0 plan_gemm, 1 plan_gemm_panel, 2 the gemm8 split-K plan; flags & 1 small_lds; bias False: a null bias; slabs: of a mode-3 launch
GemmCase = namedtuple("GemmCase", "family setting route m n k mode flags bias kernel slabs")
GEMM_CASES = []


def _add(family, setting, route, shape, mode, kernel, flags=0, bias=True, slabs=1):
    GEMM_CASES.append(GemmCase(family, setting, route, shape[0], shape[1], shape[2], mode, flags, bias and mode != 3, kernel, slabs))


# ---- tiled 128 x 128 (m < 512 or n < 512 keeps the other families out): one row, one tile, one row / column past a tile, odd N and
# N % 8 != 0 (the epilogue's 16-byte accesses need N % 8 == 0 / N % 4 == 0: element-wise otherwise), a long K; then without a bias
for bias in (True, False):
    for shape in [(1, 1, 64), (127, 129, 64), (128, 128, 64), (129, 127, 192), (77, 100, 128), (200, 77, 64), (300, 384, 1536)]:
        for mode in (0, 1, 2):
            _add("tiled", 0, 0, shape, mode, f"gemm_f16_kernel<{mode}>", bias=bias)
# ... and three of the streaming shapes below with every other family switched off
for shape in [(545, 520, 384), (512, 512, 768), (512, 8320, 128)]:
    for mode in (0, 1):
        _add("tiled", 9, 0, shape, mode, f"gemm_f16_kernel<{mode}>")

# ---- panel (route 1).  Modes 0 / 1: one tile and a one-shot chunk; TM 64 with ragged M; TM 128 (more than 256 64-row workgroups), and
# beyond 256 workgroups of 128 rows the chunk falls to 128 columns, walked kin times; N ragged in the last 64-column block; N % 8 != 0
for mode in (0, 1):
    for shape, tm in [((16, 64, 384), 64), ((65, 1152, 384), 64), ((1024, 1152, 384), 128), ((1040, 2304, 768), 128), ((100, 200, 256), 64),
                      ((64, 60, 128), 64)]:
        _add("panel", 0, 1, shape, mode, f"gemm_panel_kernel<{mode}, {tm}>")
_add("panel", 0, 1, (65, 1152, 384), 0, "gemm_panel_kernel<0, 64>", flags=1)          # small_lds: 128-column chunks, kin 3
# mode 3: 4 slabs at m <= 1024; 2 slabs of kin > 1 chunks; N ragged in the last 64-column block, and N % 4 != 0 below
PANEL3 = [((80, 384, 1536), 64, 4), ((1040, 768, 3072), 128, 2), ((96, 100, 768), 64, 2)]
for shape, tm, slabs in PANEL3:
    _add("panel", 0, 1, shape, 3, f"gemm_panel_kernel<3, {tm}>", slabs=slabs)
_add("panel", 0, 1, (80, 384, 1536), 3, "gemm_panel_kernel<3, 64>", flags=1, slabs=4)
_add("panel", 0, 1, (96, 102, 768), 3, "gemm_panel_kernel<3, 64>", slabs=2)          # (100 is a multiple of 4: this one is not)
for setting in (1, 2):                                                                 # forced chunk sizes on the K = 768 / 1536 / 3072 shapes
    for mode in (0, 1):
        _add("panel", setting, 1, (1040, 2304, 768), mode, f"gemm_panel_kernel<{mode}, 128>")
    for shape, tm, slabs in PANEL3:
        _add("panel", setting, 1, shape, 3, f"gemm_panel_kernel<3, {tm}>", slabs=slabs)
_add("panel", 3, 1, (1040, 2304, 768), 0, "gemm_panel_kernel<0, 128>")
for shape, tm, slabs in [((80, 384, 1536), 64, 4), ((1040, 768, 3072), 128, 8), ((96, 100, 768), 64, 2)]:
    _add("panel", 3, 1, shape, 3, f"gemm_panel_kernel<3, {tm}>", slabs=slabs)

# ---- gemm8, whole K, one workgroup per item: the shortest K (the prologue's two k-tiles are half the loop), half a last column
# block, several tiles; the same under the schedule variants
G8_SMALL = [(256, 256, 256), (256, 384, 384), (512, 640, 896)]
for setting, var in [(4, 0), (5, 1), (6, 2), (7, 3)]:
    for shape in G8_SMALL:
        for mode in (0, 1, 2):
            _add("gemm8", setting, 0, shape, mode, f"gemm8_kernel<{mode}, false, {var}>")
# persistent form: items just above the CU count and no multiple of it, m = 256 ceil((cus + 1) / ncb); with N = 640 a half-block item
# is followed by a full one across the item boundary, where the next item's first half tiles are issued under the last phases
for n in (640, 1024):
    ncb = (n + 255) // 256
    m = 256 * ((TABLE_CUS + 1 + ncb - 1) // ncb)
    for k in (256, 384):
        for mode in (0, 1):
            _add("gemm8p", 0, 0, (m, n, k), mode, f"gemm8_kernel<{mode}, true, 0>")

# ---- gemm8 split-K (route 2, mode 3): every slab count of kG8SplitK
for shape, slabs in [((2048, 768, 1536), 6), ((4096, 768, 768), 3), ((4096, 1024, 512), 2), ((2048, 512, 2048), 8), ((2048, 1024, 1024), 4)]:
    _add("gemm8sk", 0, 2, shape, 3, "gemm8_kernel<3, false, 0>", slabs=slabs)

# ---- big: 16 / 18 / 26 / 20 k-steps of 32 against four stages; ragged M
for shape in [(257, 256, 512), (300, 512, 576), (256, 256, 832), (511, 768, 640)]:
    for mode in (0, 1):
        _add("big", 8, 0, shape, mode, f"gemm_big_kernel<{mode}, 256>")
for mode in (0, 1):
    _add("big", 0, 0, (4100, 2048, 512), mode, f"gemm_big_kernel<{mode}, 256>")

# ---- stream: every resident K; a ragged last 32-row tile with 8 live columns in the last column block and uneven tiles per stream; 65
# column blocks (fewer than 8 streams: the `nstreams & 7` indexing branch); the K = 768 split
for k in (128, 256, 384, 512):
    for shape in [(512, 512, k), (545, 520, k)]:
        for mode in (0, 1):
            _add("stream", 0, 0, shape, mode, f"gemm_stream_kernel<{k}, {mode}>")
for mode in (0, 1):
    _add("stream", 0, 0, (512, 8320, 128), mode, f"gemm_stream_kernel<128, {mode}>")
    for shape in [(512, 512, 768), (545, 520, 768), (2049, 1152, 768)]:
        _add("streamks", 0, 0, shape, mode, f"gemm_stream_ks_kernel<768, {mode}>")


# ---- projection + LayerNorm (crs_proj_ln_f16): kernels = the describe lines' kernels in launch order
ProjLnCase = namedtuple("ProjLnCase", "setting tokens hidden k flags big_ln kernels slabs")
PROJ_LN_CASES = []
for setting, ring in [(0, "gemm_rowln2_kernel<64, 2>"), (10, "gemm_rowln2_kernel<32, 4>")]:
    for tokens in (4097, 4224):                       # one row, and nothing, past the last whole 128-row block... of 33 blocks
        for k in (192, 384, 1536):
            PROJ_LN_CASES.append(ProjLnCase(setting, tokens, 384, k, 0, True, (ring,), 1))
PROJ_LN_CASES += [
    ProjLnCase(0, 80, 384, 1536, 0, False, ("gemm_panel_kernel<3, 64>", "layernorm2_kernel<3, 4>"), 4),
    ProjLnCase(0, 2048, 768, 3072, 0, False, ("gemm_panel_kernel<3, 128>", "layernorm2_kernel<6, 2>"), 2),
    ProjLnCase(0, 4096, 768, 768, 0, False, ("gemm8_kernel<3, false, 0>", "layernorm2_kernel<6, 3>"), 3),
    ProjLnCase(0, 300, 320, 1280, 0, False, ("gemm_f16_kernel<2>", "layernorm_kernel<16, 1>"), 1),
]


def gemm_id(c):
    return f"{c.family}-r{c.route}-{c.m}x{c.n}x{c.k}-m{c.mode}" + ("-small" if c.flags else "") + ("" if c.bias or c.mode == 3 else "-nobias")


def proj_ln_id(c):
    return f"{c.tokens}x{c.hidden}x{c.k}-" + ("big" if c.big_ln else "small")


def grid_of(line):
    """(gx, gy, gz) of a describe line"""
    return tuple(int(v) for v in re.search(r" grid=(\d+)x(\d+)x(\d+) ", line).groups())


def slab_factor(c, line):
    """the slab count a mode-3 describe line shows: the panel's grid z; gemm8's items over its 256 x 256 tiles"""
    gx, gy, gz = grid_of(line)
    return gz if c.route == 1 else gx // ((c.m // 256) * (c.n // 256))


# ---- one fresh child process per knob setting (the knobs are read once per process) ----------------------------------------------------
CHILD_ENV = "GEMM_CASES_SETTING"          # set in a child: the index of its setting; the parent process runs setting 0
RATIO_TAG = "gemm-ratio"                  # the tests print "gemm-ratio <family> mode <m> <err / bound> <case id>" per case
_failed = []


def setting_here():
    return int(os.environ.get(CHILD_ENV, "0"))


def run_setting_child(test_file, si, select, n_cases, timeout=300):
    """pytest on test_file in a fresh process under SETTINGS[si], selecting the case test `select`; returns the number of cases the
    child skipped (a device the table was not written for).  After a child failed no further child is started."""
    import pytest
    if _failed:
        pytest.fail(f"not started: the child of setting {SETTINGS[_failed[0]]} failed")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **SETTINGS[si])
    env[CHILD_ENV] = str(si)
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider", test_file, "-k", select],
                           cwd=root, env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _failed.append(si)
        raise
    print("".join(line[line.index(RATIO_TAG):] + "\n" for line in r.stdout.splitlines() if RATIO_TAG in line), end="")   # (behind pytest's dots)
    if r.returncode != 0:
        _failed.append(si)
    assert r.returncode == 0, str(SETTINGS[si]) + r.stdout[-3000:] + r.stderr[-2000:]
    tail = r.stdout.strip().splitlines()[-1]
    passed = int((re.search(r"(\d+) passed", tail) or [0, 0])[1])
    skipped = int((re.search(r"(\d+) skipped", tail) or [0, 0])[1])
    assert passed + skipped == n_cases, (SETTINGS[si], tail)       # the child ran exactly this setting's cases
    return skipped
