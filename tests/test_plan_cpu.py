"""No GPU: the scan planner (csrc/plan.cpp, csrc/scan_forms.h) as the stand-alone program tools/plan_table.cpp, built here with g++.

1. Against tests/golden/scan_plans.json.xz -- crs_scan_plan_describe and crs_scan_workspace_bytes recorded on an MI355X before the
   planner became a pure function, one fresh process per knob setting -- the planner reproduces every text (up to the
   "; cert tail:" suffix, which finish.hip decides) and every byte count.
2. Every plan it returns over all row lengths, the golden's query counts and shard sizes and every k satisfies its family's
   form_exists, the predicate the launch ladders of the scan_*.hip files take their `if constexpr` conditions from.
3. The launch arguments the describe text never showed (ticket, t_dyn, dyn_mask, nt, boot, stagger, MFMA shape), on cases worked
   out by hand from the code as it stood before; each derivation is in its test's docstring."""
import itertools
import json
import lzma
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "compressed-rag-suite_amd", "csrc")
COLS = ("family waves slots tile_rows n_tiles streams qblocks kp nt ticket t_dyn dyn_mask boot sched no_stagger mfma form_exists "
        "workspace_bytes text").split()
F16, I8 = 0, 1


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_table")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "plan_table.cpp"),
                    os.path.join(CSRC, "plan.cpp")], check=True, timeout=300)

    def run(cases, cus=256, env=None):
        """cases: (nq, dim, k, n_rows, slab_type) -> one dict per case (ints but for family and text)"""
        e = {k: v for k, v in os.environ.items() if not k.startswith("CRS_")}
        e.update(env or {})
        out = subprocess.run([exe, str(cus)], input="".join("%d %d %d %d %d\n" % c for c in cases), env=e, capture_output=True,
                             text=True, check=True, timeout=120).stdout.splitlines()
        assert len(out) == len(cases)
        rows = []
        for c, line in zip(cases, out):
            f = line.split("\t")
            assert len(f) == len(COLS), (c, line)
            rows.append({n: (v if n in ("family", "text") else int(v)) for n, v in zip(COLS, f)})
        return rows
    return run


@pytest.fixture(scope="module")
def golden():
    with lzma.open(os.path.join(ROOT, "tests", "golden", "scan_plans.json.xz"), "rt") as f:
        g = json.load(f)
    assert g["order"] == ["slab_type", "dim", "nq", "k", "n_rows"]
    return g


def grid_cases(grid):
    return [(nq, dim, k, n, st) for st, dim, nq, k, n in
            itertools.product(grid["slab_type"], grid["dim"], grid["nq"], grid["k"], grid["n_rows"])]


def test_golden_covers_the_grid_and_the_settings(golden):
    g = golden["grid"]
    assert g["dim"] == [128, 256, 384, 512, 640, 768, 896, 1024] and g["slab_type"] == [0, 1]
    assert g["nq"] == [1, 64, 65, 128, 129, 256, 512]
    assert g["k"] == [1, 4, 5, 10, 11, 16, 17, 24, 25, 32, 33, 40, 41, 48, 49, 56, 57, 64]
    assert g["n_rows"] == [1, 31, 4096, 300_000, 1_250_000, 10_000_000]
    assert [s["env"] for s in golden["settings"]] == [
        {}, {"CRS_SCAN_TB": "0"}, {"CRS_SCAN_WIDE": "0"}, {"CRS_SCAN_W1": "0"}, {"CRS_SCAN_LONG_CHAIN": "0"}, {"CRS_SCAN_NT": "0"},
        {"CRS_SCAN_NT": "1"}, {"CRS_SCAN_SHARE_TAU": "1"}]
    n = len(grid_cases(g))
    for s in golden["settings"]:
        assert len(s["text"]) == n and len(s["bytes"]) == n // 2
    # every family is in the default table
    names = {golden["texts"][i].split("<")[0] for i in golden["settings"][0]["text"]}
    assert names == {"scan_f16_kernel", "scan_i8_kernel", "scan_tb_kernel", "scan_wide_kernel", "scan_w2_kernel"}


@pytest.mark.parametrize("setting", range(8))
def test_planner_reproduces_the_golden_table(table, golden, setting):
    s = golden["settings"][setting]
    cases = grid_cases(golden["grid"])
    rows = table(cases, cus=golden["cus"], env=s["env"])
    half = len(cases) // 2
    bad = []
    for i, (c, r) in enumerate(zip(cases, rows)):
        want = golden["texts"][s["text"][i]]
        assert "; cert tail: " in want
        want_bytes = golden["sizes"][s["bytes"][i % half]]   # the byte count does not depend on the slab type
        if r["text"] != want.split("; cert tail: ")[0] or r["workspace_bytes"] != want_bytes:
            bad.append((c, r["text"], r["workspace_bytes"], want, want_bytes))
    assert not bad, "%d of %d cases differ under %s, first: %s" % (len(bad), len(cases), s["env"], bad[:3])


@pytest.mark.parametrize("env", [{}, {"CRS_SCAN_TB": "0"}, {"CRS_SCAN_WIDE": "0"}, {"CRS_SCAN_W1": "0"}, {"CRS_SCAN_LONG_CHAIN": "0"},
                                 {"CRS_WIDE_MFMA": "16"}, {"CRS_WIDE_MFMA": "32"}], ids=str)
def test_every_plan_is_a_form_the_launch_ladders_hold(table, golden, env):
    g = golden["grid"]
    cases = [(nq, pdim, k, n, st) for st, pdims in ((F16, range(128, 1025, 128)), (I8, range(256, 1025, 256)))
             for pdim in pdims for nq in g["nq"] for k in range(1, 65) for n in g["n_rows"]]
    seen, few_streams, short_shard = set(), 0, 0
    for cus in (256, 4):    # 4 CUs: fewer than 8 streams under several query blocks
        rows = table(cases, cus=cus, env=env)
        bad = [(c, r) for c, r in zip(cases, rows) if r["form_exists"] != 1]
        assert not bad, "%d plans name a form that does not exist, first: %s" % (len(bad), bad[:3])
        for c, r in zip(cases, rows):
            seen.add((r["family"], c[4]))
            assert 1 <= r["streams"] <= r["n_tiles"] and r["qblocks"] >= 1 and r["kp"] >= 1, (c, r)
            few_streams += r["qblocks"] > 1 and r["streams"] < 8
            short_shard += r["n_tiles"] < cus and r["streams"] == r["n_tiles"]
    assert few_streams and short_shard
    if not env:
        assert seen == {("Classic", F16), ("Classic", I8), ("TileBest", F16), ("TileBest", I8), ("Wide", F16), ("W1", F16)}


C4 = (64, 384, 24, 10_000_000, F16)


def test_long_chain_on_the_large_shard(table):
    """10 M x 384 fp16, 64 queries, k 24, 256 CUs.  One query block of 64, so 4 waves; scan_tb.hip's tiles are 32 rows at 384
    elements: ceil(10 M / 32) = 312 500 tiles; 2 workgroups per CU: 512 streams.  611 tiles per stream is no dump (611 x 512 >
    8192), k > 16 takes the long chain, 24 slots at k 24, kp = 24.  The slab is 7.68 GB >= 1 GiB with one query block: nt.
    floor(312 500 / 512) = 610 rounds >= 96: ticketed; static rounds floor(610 x 15 / 100) = 91, t_dyn = 91 x 512 = 46 592; 8 tiles
    per ticket: dyn_mask 7.  610 rounds >= 24: no bootstrap."""
    r, = table([C4])
    assert (r["family"], r["waves"], r["slots"], r["tile_rows"], r["n_tiles"], r["streams"], r["qblocks"], r["kp"]) == \
        ("TileBest", 4, 24, 32, 312_500, 512, 1, 24)
    assert (r["nt"], r["boot"], r["ticket"], r["t_dyn"], r["dyn_mask"], r["sched"], r["mfma"]) == (1, 0, 1, 46_592, 7, 2, 0)
    # percent 0 is the static stride; 50 % in granules of 4: floor(610 / 2) = 305 static rounds
    r, = table([C4], env={"CRS_TB_DYN": "0"})
    assert (r["ticket"], r["t_dyn"], r["dyn_mask"]) == (0, 312_500, 0)
    r, = table([C4], env={"CRS_TB_DYN": "50", "CRS_TB_DYN_G": "4"})
    assert (r["ticket"], r["t_dyn"], r["dyn_mask"]) == (1, 305 * 512, 3)


def test_two_query_blocks_take_no_ticket(table):
    """The same shard with 128 queries and scan_wide.hip off: k 24 > 16 keeps 4 waves = 64 queries per workgroup, two query
    blocks share the 512 resident workgroups: 256 streams (a multiple of 8), the 24-slot chain again; the ticket and the nt stream
    are for one query block only.  With scan_wide.hip on, 512 queries are two blocks of its 8-wave form (64-row tiles, one
    workgroup per CU: 128 streams, kp = 2 x 24): no ticket, no nt either."""
    r, = table([(128,) + C4[1:]], env={"CRS_SCAN_WIDE": "0"})
    assert (r["family"], r["waves"], r["slots"], r["streams"], r["qblocks"]) == ("TileBest", 4, 24, 256, 2)
    assert (r["nt"], r["ticket"], r["t_dyn"], r["dyn_mask"]) == (0, 0, 312_500, 0)
    r, = table([(512,) + C4[1:]])
    assert (r["family"], r["waves"], r["slots"], r["tile_rows"], r["n_tiles"], r["streams"], r["qblocks"], r["kp"]) == \
        ("Wide", 8, 24, 64, 156_250, 128, 2, 48)
    assert (r["nt"], r["ticket"], r["t_dyn"]) == (0, 0, 156_250)


def test_int8_rows_of_1024_elements_take_no_ticket(table):
    """10 M int8 rows, 64 queries, k 10: scan_i8.hip's 10-slot chain on 512 streams of 32-row tiles (610 rounds).  768-element rows
    are ticketed like the fp16 case above; 1024-element rows stay static (those instantiations spill)."""
    a, b = table([(64, 768, 10, 10_000_000, I8), (64, 1024, 10, 10_000_000, I8)])
    assert (a["family"], a["slots"], a["streams"], a["kp"], a["nt"]) == ("TileBest", 10, 512, 10, 1)
    assert (a["ticket"], a["t_dyn"], a["dyn_mask"]) == (1, 46_592, 7)
    assert (b["family"], b["slots"], b["streams"], b["kp"], b["nt"]) == ("TileBest", 10, 512, 10, 1)
    assert (b["ticket"], b["t_dyn"], b["dyn_mask"]) == (0, 312_500, 0)


def test_ticket_on_a_short_stream_when_asked(table):
    """300 000 x 128 fp16, 64 queries, k 16: 9375 tiles of 32 rows, 3 workgroups per CU at 128 elements: 768 streams, 13 tiles
    per stream (13 x 768 > 8192: chain of 16).  floor(9375 / 768) = 12 rounds < 96: static by default; CRS_TB_DYN_MIN=4 tickets it:
    floor(12 x 15 / 100) = 1 static round is raised to the minimum of 2, t_dyn = 2 x 768.  12 rounds < 24 sets the bootstrap flag
    (read by scan.hip only).  The slab is 77 MB: no nt."""
    case = (64, 128, 16, 300_000, F16)
    r, = table([case])
    assert (r["family"], r["waves"], r["slots"], r["n_tiles"], r["streams"], r["kp"]) == ("TileBest", 4, 16, 9375, 768, 16)
    assert (r["nt"], r["ticket"], r["t_dyn"], r["boot"]) == (0, 0, 9375, 1)
    r, = table([case], env={"CRS_TB_DYN_MIN": "4"})
    assert (r["ticket"], r["t_dyn"], r["dyn_mask"]) == (1, 1536, 7)
    r, = table([case], env={"CRS_TB_DYN_MIN": "0", "CRS_TB_DYN": "100"})   # the floor of 4 rounds; 0 static rounds raised to 2
    assert (r["ticket"], r["t_dyn"]) == (1, 1536)


def test_wide_streamed_form_ticket_stagger_and_shape(table):
    """10 M x 384 fp16, 256 queries, k 24: scan_wide.hip with 8 waves (more than 128 queries) = 256 queries per workgroup, one
    block; 64-row tiles: 156 250; one workgroup per CU: 256 streams; 24 slots per lane pair, kp = 48.  24 slots is a streamed
    form: nt (7.68 GB), and floor(156 250 / 256) = 610 rounds: 91 static, t_dyn = 91 x 256 = 23 296, dyn_mask 7.  <384, 8, 24> exists
    in both MFMA shapes and 384-element rows default to 16x16x32.  The knobs: CRS_WIDE_DYN=0 static, CRS_WIDE_MFMA=32 the other
    shape, CRS_WIDE_STAGGER=0 sets no_stagger.  k 16 (16 slots) is not streamed: no nt, no ticket, 32x32x16 only whatever the knob."""
    case = (256, 384, 24, 10_000_000, F16)
    r, = table([case])
    assert (r["family"], r["waves"], r["slots"], r["tile_rows"], r["n_tiles"], r["streams"], r["qblocks"], r["kp"]) == \
        ("Wide", 8, 24, 64, 156_250, 256, 1, 48)
    assert (r["nt"], r["ticket"], r["t_dyn"], r["dyn_mask"], r["no_stagger"], r["mfma"]) == (1, 1, 23_296, 7, 0, 16)
    r, = table([case], env={"CRS_WIDE_DYN": "0", "CRS_WIDE_MFMA": "32", "CRS_WIDE_STAGGER": "0"})
    assert (r["nt"], r["ticket"], r["t_dyn"], r["dyn_mask"], r["no_stagger"], r["mfma"]) == (1, 0, 156_250, 0, 1, 32)
    r, = table([(256, 384, 16, 10_000_000, F16)], env={"CRS_WIDE_MFMA": "16"})
    assert (r["family"], r["slots"], r["kp"], r["nt"], r["ticket"], r["mfma"]) == ("Wide", 16, 32, 0, 0, 32)
    r, = table([(256, 256, 32, 10_000_000, F16)])    # 256-element rows stay on 32x32x16 by default
    assert (r["family"], r["slots"], r["mfma"]) == ("Wide", 32, 32)


def test_w1_hands_over_past_its_dump_limit(table):
    """768-element fp16 rows, 256 queries, k 10, 256 CUs: scan_w1.hip (256 queries per workgroup, one workgroup per CU: 256 streams
    of 32-row tiles) dumps every tile: kp = tiles per stream, at most 256, i.e. 256 x 256 x 32 = 2 097 152 rows.  One row more
    and the 8-wave tile-best chain takes over (k <= 16 and more than 64 queries: 8 waves = 128 queries per workgroup, two blocks;
    16-row tiles at 768 elements: 131 073; one workgroup per CU over two blocks: 128 streams; chain of 10).  Two blocks: no
    ticket and no nt, though the slab is 3.2 GB."""
    a, b = table([(256, 768, 10, 2_097_152, F16), (256, 768, 10, 2_097_153, F16)])
    assert (a["family"], a["waves"], a["tile_rows"], a["n_tiles"], a["streams"], a["qblocks"], a["kp"]) == ("W1", 8, 32, 65_536, 256, 1, 256)
    assert (a["nt"], a["ticket"]) == (0, 0) and a["text"].startswith("scan_w2_kernel<768> (256 queries/workgroup, dump)")
    assert (b["family"], b["waves"], b["slots"], b["tile_rows"], b["n_tiles"], b["streams"], b["qblocks"], b["kp"]) == \
        ("TileBest", 8, 10, 16, 131_073, 128, 2, 10)
    assert (b["nt"], b["ticket"], b["t_dyn"]) == (0, 0, 131_073)


def test_classic_through_the_fall_through(table):
    """300 000 x 512 fp16, 64 queries, k 64: tile-best is tried first (9375 tiles on 512 streams: 19 per stream, 9728 candidates
    > 8192: no dump) and has no chain for k 64 at 512 elements (48 slots at most), so the threshold kernel takes it: the same
    512 streams, kp = k, no refine.  floor(9375 / 512) = 18 rounds < 24: bootstrap, unless CRS_SCAN_BOOT=0.  k 48 stays tile-best."""
    case = (64, 512, 64, 300_000, F16)
    r, = table([case])
    assert (r["family"], r["slots"], r["tile_rows"], r["streams"], r["kp"], r["nt"], r["ticket"], r["boot"], r["sched"]) == \
        ("Classic", -1, 32, 512, 64, 0, 0, 1, 2)
    assert r["text"] == "scan_f16_kernel<512,32,32> streams=512 qblocks=1 kp=64 + merge"
    r, = table([case], env={"CRS_SCAN_BOOT": "0", "CRS_SCAN_SCHED": "1"})
    assert (r["family"], r["boot"], r["sched"]) == ("Classic", 0, 1)
    r, = table([(64, 512, 48, 300_000, F16)])
    assert (r["family"], r["slots"], r["kp"]) == ("TileBest", 48, 48)
