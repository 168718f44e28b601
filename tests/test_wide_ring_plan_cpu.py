"""No GPU: the plan fields of the wide kernel's ring form (csrc/scan_wide.hip, "Ring form"; csrc/scan_forms.h wide_ring_form), read
through tools/plan_table.cpp --ring (ring, lds, ticket, t_dyn, dyn_mask, describe text) beside its default columns.

  * ring is true for (384-element rows, 8 waves, 24 slots, MFMA shape 16) and for no other plan, over every row length, the query
    counts that reach every family, every k up to 40, two shard sizes and both slab types;
  * the launch's LDS bytes: three 48 KB tile buffers = 147 456 for the ring form; two buffers, or one buffer and the 4 KB per wave of
    the query transpose, for every other wide plan (worked out by hand below); 0 for the other families;
  * CRS_WIDE_RING=0 flips both, CRS_WIDE_MFMA=32 too (the 32x32x16 kernel of the form has no ring);
  * the describe text does not show the choice;
  * the ring looks two tiles ahead, so its plans keep three static rounds where the others keep two."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "compressed-rag-suite_amd", "csrc")
COLS = ("family waves slots tile_rows n_tiles streams qblocks kp nt ticket t_dyn dyn_mask boot sched no_stagger mfma form_exists "
        "workspace_bytes text").split()
RCOLS = "ring lds ticket t_dyn dyn_mask text".split()
F16, I8 = 0, 1
C4X4 = (256, 384, 24, 10_000_000, F16)      # the flagship's sweep: four 64-query batches in one launch
TEXT = "scan_wide_kernel<384,8,24> streams=256 qblocks=1 kp=48 nt + merge + refine"


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ringplan") / "plan_table")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "plan_table.cpp"),
                    os.path.join(CSRC, "plan.cpp")], check=True, timeout=300)

    def run(cases, env=None, cus=256):
        """cases: (nq, dim, k, n_rows, slab_type) -> one dict per case: the default columns and the --ring columns"""
        e = {k: v for k, v in os.environ.items() if not k.startswith("CRS_")}
        e.update(env or {})
        text = "".join("%d %d %d %d %d\n" % c for c in cases)
        both = []
        for args, cols in (([str(cus)], COLS), (["--ring", str(cus)], RCOLS)):
            out = subprocess.run([exe] + args, input=text, env=e, capture_output=True, text=True, check=True, timeout=120).stdout.splitlines()
            assert len(out) == len(cases)
            rows = []
            for c, line in zip(cases, out):
                f = line.split("\t")
                assert len(f) == len(cols), (c, line)
                rows.append({n: (v if n in ("family", "text") else int(v)) for n, v in zip(cols, f)})
            both.append(rows)
        merged = []
        for a, b in zip(*both):
            assert (a["text"], a["ticket"], a["t_dyn"], a["dyn_mask"]) == (b["text"], b["ticket"], b["t_dyn"], b["dyn_mask"])
            merged.append({**a, "ring": b["ring"], "lds": b["lds"]})
        return merged
    return run


def test_ring_for_the_flagship_form_only(table):
    cases = [(nq, pdim, k, n, st) for st, pdims in ((F16, range(128, 1025, 128)), (I8, range(256, 1025, 256)))
             for pdim in pdims for nq in (1, 64, 65, 128, 129, 256, 512) for k in range(1, 41) for n in (4096, 10_000_000)]
    rows = table(cases)
    on = 0
    for c, r in zip(cases, rows):
        want = r["family"] == "Wide" and (c[1], r["waves"], r["slots"], r["mfma"]) == (384, 8, 24, 16)
        assert r["ring"] == int(want), (c, r)
        on += want
        if r["family"] != "Wide":
            assert r["lds"] == 0, (c, r)
    # 384-element fp16 rows, 129+ queries, k 17 .. 24, both shard sizes
    assert on == 3 * 8 * 2


def test_lds_bytes_follow_the_choice(table):
    """Tile bytes = tile rows x row elements x 2; the prologue's query transpose takes 4 KB per wave in the last buffer.
    <384, 8>: 64-row tiles of 49 152 bytes: ring 3 x 49 152 = 147 456, else 2 x 49 152 = 98 304 (> 49 152 + 32 768).
    <256, 8>: 32 768-byte tiles: 65 536.  <128, 8>: 16 384-byte tiles: two buffers are 32 768, one buffer + 32 768 of transpose is
    49 152.  <384, 4>: 32-row tiles of 24 576 bytes: 49 152 (> 24 576 + 16 384).  <512, 8>: 32-row tiles of 32 768 bytes: 65 536."""
    r, = table([C4X4])
    assert (r["family"], r["waves"], r["slots"], r["mfma"], r["ring"], r["lds"]) == ("Wide", 8, 24, 16, 1, 147_456)
    assert r["text"] == TEXT
    got = table([(256, 384, 32, 10_000_000, F16), (256, 384, 16, 10_000_000, F16), (256, 256, 24, 10_000_000, F16),
                 (256, 128, 24, 10_000_000, F16), (128, 384, 24, 10_000_000, F16), (256, 512, 10, 10_000_000, F16)])
    assert [(x["waves"], x["ring"], x["lds"]) for x in got] == [(8, 0, 98_304), (8, 0, 98_304), (8, 0, 65_536), (8, 0, 49_152), (4, 0, 49_152),
                                                               (8, 0, 65_536)]


@pytest.mark.parametrize("env", [{"CRS_WIDE_RING": "0"}, {"CRS_WIDE_MFMA": "32"}], ids=str)
def test_knobs_select_the_two_buffer_kernel(table, env):
    r, = table([C4X4], env=env)
    assert (r["family"], r["waves"], r["slots"], r["ring"], r["lds"]) == ("Wide", 8, 24, 0, 98_304)
    assert r["mfma"] == (32 if "CRS_WIDE_MFMA" in env else 16)
    assert r["text"] == TEXT                      # the describe text never shows the choice
    d, = table([C4X4])
    for col in COLS:                              # and nothing else of the default plan moves with CRS_WIDE_RING
        if "CRS_WIDE_RING" in env or col != "mfma":
            assert r[col] == d[col], col


def test_ring_plans_keep_three_static_rounds(table):
    """10 M x 384, 256 queries, k 24: 156 250 tiles on 256 streams, 610 rounds; 15 % static: 91 rounds, t_dyn = 23 296 whatever the
    ring.  CRS_TB_DYN=100 asks for no static round: the two-buffer kernels are given 2 (t_dyn = 512), the ring kernel, which knows
    its first THREE tiles without a ticket, 3 (t_dyn = 768)."""
    r, = table([C4X4])
    assert (r["ring"], r["ticket"], r["t_dyn"], r["dyn_mask"]) == (1, 1, 23_296, 7)
    r, = table([C4X4], env={"CRS_TB_DYN": "100"})
    assert (r["ring"], r["ticket"], r["t_dyn"]) == (1, 1, 768)
    r, = table([C4X4], env={"CRS_TB_DYN": "100", "CRS_WIDE_RING": "0"})
    assert (r["ring"], r["ticket"], r["t_dyn"]) == (0, 1, 512)
    r, = table([C4X4], env={"CRS_TB_DYN": "100", "CRS_WIDE_MFMA": "32"})
    assert (r["ring"], r["ticket"], r["t_dyn"]) == (0, 1, 512)
