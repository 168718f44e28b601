"""No GPU: the case table of tests/_scan_form_cases.py is closed over the scan kernel instantiations that exist.

tools/plan_table.cpp, built here with g++, lists the forms from the predicates of csrc/scan_forms.h (`--forms`) and plans every
shape under its leg's knobs.  The table must name exactly the listed forms and be what tools/make_scan_form_cases.py finds, each
case (its smallest-k twin, its second shapes) must plan to its form, the legs must partition the table, and every register
chain must meet a stream longer than itself -- so a form added to scan_forms.h without a case, or a planner change that moves
a case to another kernel or empties a chain, fails here before a GPU is involved.  The planted corpus is checked on its fp64
reference alone; tests/test_scan_forms_gpu.py runs the cases."""
import collections
import importlib.util
import json
import lzma
import os
import subprocess

import numpy as np
import pytest

import _scan_form_cases as fc
from topk_check import BAND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "compressed-rag-suite_amd", "csrc")
F16, I8 = fc.F16, fc.I8
MAX_K = 64      # CRS_MAX_K (include/crs_hip.h)

_spec = importlib.util.spec_from_file_location("make_scan_form_cases", os.path.join(ROOT, "tools", "make_scan_form_cases.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("forms") / "plan_table")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", path, os.path.join(ROOT, "tools", "plan_table.cpp"),
                    os.path.join(CSRC, "plan.cpp")], check=True, timeout=300)
    return path


@pytest.fixture(scope="module")
def cus():
    with lzma.open(os.path.join(ROOT, "tests", "golden", "scan_plans.json.xz"), "rt") as f:
        n = json.load(f)["cus"]
    assert n == fc.CUS == gen.CUS
    return n


def plan(exe, cus, cases, env):
    return gen.plan(exe, cases, env, cus)


def shapes_of(name):
    """every shape the device test runs for a form: (nq, n_rows, leg, what)"""
    nq, dim, k, n, st, leg = fc.CASES[name]
    out = [(nq, n, leg, "case")]
    out += [fc.BOOT_ABOVE[name] + (leg, "above the bootstrap")] if name in fc.BOOT_ABOVE else []
    out += [fc.MULTI_BLOCK[name] + (leg, "two query blocks")] if name in fc.MULTI_BLOCK else []
    out += [fc.LONG_STREAM[name] + ("long stream",)] if name in fc.LONG_STREAM else []
    return out


@pytest.fixture(scope="module")
def plans(exe, cus):
    """{(form, nq, n_rows): plan at the form's largest k} for every shape of every form"""
    out = {}
    for leg, env in fc.LEGS.items():
        todo = [(name, nq, n) for name in fc.CASES for nq, n, l, _ in shapes_of(name) if l == leg]
        cases = [(nq, fc.CASES[name][1], fc.CASES[name][2], n, fc.CASES[name][4]) for name, nq, n in todo]
        out.update(zip(todo, plan(exe, cus, cases, env)))
    return out


def test_the_case_table_names_exactly_the_forms_that_exist(exe):
    forms = gen.list_forms(exe)
    assert len(forms) == len(set(forms))
    assert set(fc.CASES) == set(forms), (sorted(set(forms) - set(fc.CASES)), sorted(set(fc.CASES) - set(forms)))
    print("%d forms: %s" % (len(forms), dict(collections.Counter(fc.family(f) for f in forms))))
    assert len(forms) == 166      # at this commit; a new form needs a case AND this count


def test_the_tables_are_what_the_generator_gives(exe):
    """tools/make_scan_form_cases.py states the rules by which every shape was chosen (smallest rung of the ladder, largest k,
    one query block, the first leg that reaches the form) and searches the planner by them: the committed tables are its answer."""
    got = gen.generate(exe)
    for table in ("CASES", "BOOT_ABOVE", "MULTI_BLOCK", "LONG_STREAM"):
        assert got[table] == getattr(fc, table), table
    assert list(got["CASES"]) == list(fc.CASES)      # and in the listing's order: forms of one row length share their rows
    assert dict(gen.LEGS) == dict(fc.LEGS)


def test_the_legs_partition_the_table():
    by_leg = {leg: fc.leg_names(leg) for leg in fc.LEGS}
    assert sum(len(v) for v in by_leg.values()) == len(fc.CASES)
    assert set().union(*map(set, by_leg.values())) == set(fc.CASES)
    assert {leg: len(v) for leg, v in by_leg.items()} == {"default": 118, "CRS_SCAN_TB=0": 24, "CRS_SCAN_WIDE=0": 16,
                                                          "CRS_SCAN_W1=0": 4, "CRS_WIDE_MFMA=16": 2, "CRS_WIDE_MFMA=32": 2}
    # every threshold form, and nothing else, runs with the tile-best kernels off; the staging-variant legs run the fp16 ones
    assert set(by_leg["CRS_SCAN_TB=0"]) == {n for n in fc.CASES if fc.is_classic(n)}
    assert sum(fc.family(n) == "scan_f16" for n in by_leg["CRS_SCAN_TB=0"]) == 16
    # every long-stream shape has a process: its form's own, or a child leg's (none needs the test process from a child)
    elsewhere = {p: fc.long_streams_from_elsewhere(p) for p in ("default",) + fc.CHILD_LEGS}
    assert not elsewhere["default"] and not elsewhere["CRS_SCAN_TB=0"]
    own = [n for n, v in fc.LONG_STREAM.items() if fc.process_of(v[2]) == fc.process_of(fc.CASES[n][5])]
    assert len(own) + sum(map(len, elsewhere.values())) == len(fc.LONG_STREAM)


@pytest.mark.parametrize("leg", list(fc.LEGS))
def test_every_case_plans_to_its_form(exe, cus, plans, leg):
    names = fc.leg_names(leg)
    for name in names:
        nq, dim, k, n, st, _ = fc.CASES[name]
        r = plans[(name, nq, n)]
        assert r["name"] == name and r["form_exists"] == 1, (name, r)
        assert r["text"].startswith(name.split("/")[0])
        # what the device test takes from the name and the describe text is what the planner holds
        assert r["tile_rows"] == fc.tile_rows_of(name) and fc.parse_plan(r["text"]) == (r["streams"], r["qblocks"], r["kp"])
        # ragged: no multiple of 64, the last partial tile inside the shard; a query count that fills no wave exactly
        assert n % 64 and n % r["tile_rows"] >= 3 and r["n_tiles"] * r["tile_rows"] > n and nq % 16
        assert dim == fc.template_args(name)[0] and r["qblocks"] == 1
        if fc.is_dump(name):
            assert -(-r["n_tiles"] // r["streams"]) >= 3 and r["n_tiles"] % r["streams"]     # streams of unequal length
    # k is the largest that selects the form
    more = [(n, fc.CASES[n][:2] + (fc.CASES[n][2] + 1,) + fc.CASES[n][3:5]) for n in names if fc.CASES[n][2] < MAX_K]
    for (name, c), r in zip(more, plan(exe, cus, [c for _, c in more], fc.LEGS[leg])):
        assert r["name"] != name, (name, c)
    # the smallest-k twin of the dump and threshold forms is the same form
    twins = [(n, fc.CASES[n][:2] + (fc.twin_k(n),) + fc.CASES[n][3:5]) for n in names if fc.twin_k(n) is not None]
    for (name, c), r in zip(twins, plan(exe, cus, [c for _, c in twins], fc.LEGS[leg])):
        assert r["name"] == name and r["form_exists"] == 1, (name, c, r)
    if leg == "default":
        assert len(twins) == 8 + 1 + 4 + 1      # dump forms: scan_tb with 4 waves, with 8 (1024-element rows), scan_i8, scan_w2
    if leg == "CRS_SCAN_TB=0":
        assert len(twins) == 24


def test_the_second_shapes_plan_to_the_same_form(plans):
    for name in fc.CASES:
        for nq, n, leg, what in shapes_of(name)[1:]:
            r = plans[(name, nq, n)]
            assert r["name"] == name and r["form_exists"] == 1 and r["tile_rows"] == fc.tile_rows_of(name), (name, what, r)
            assert n % 64 and n % r["tile_rows"] >= 3 and nq % 16, (name, what)
    assert set(fc.BOOT_ABOVE) == {n for n in fc.CASES if fc.family(n) == "scan_f16" and fc.template_args(n)[1:] == [32, 16]}
    for name, (nq, n) in fc.BOOT_ABOVE.items():
        assert (plans[(name,) + fc.CASES[name][0:4:3]]["boot"], plans[(name, nq, n)]["boot"]) == (1, 0)
    # the 8-wave wide forms again: two query blocks, streams long enough to fill a 16-slot parity list and a 32-slot split list
    assert set(fc.MULTI_BLOCK) == {n for n in fc.CASES if fc.family(n) == "scan_wide" and fc.template_args(n)[1] == 8}
    for name, (nq, n) in fc.MULTI_BLOCK.items():
        r = plans[(name, nq, n)]
        assert r["qblocks"] == 2 and r["n_tiles"] // r["streams"] >= 32


def test_every_register_chain_fills_and_overflows(plans):
    """Every scan_tb / scan_i8 chain form has a shape -- its case, or its long-stream shape -- at which EVERY workgroup sees more
    tiles than the chain has slots, so each slot holds a tile and the tail falls off; the planted chain there has more winners
    than slots too (64 at most: the 64-slot chain takes exactly 64, with other tiles behind them)."""
    chains = [n for n in fc.CASES if fc.chain_slots(n)]
    assert len(chains) == 83 and len(fc.LONG_STREAM) == 45 and set(fc.LONG_STREAM) <= set(chains)
    for name in chains:
        nq, n = fc.LONG_STREAM[name][:2] if name in fc.LONG_STREAM else fc.CASES[name][0:4:3]
        r, slots = plans[(name, nq, n)], fc.chain_slots(name)
        assert r["n_tiles"] // r["streams"] > slots, (name, r["n_tiles"], r["streams"])
        p = fc.plant_positions(n, r["tile_rows"], r["streams"], nq, fc.chain_stride(name))
        winners = [len(rows) for kind, rows in p.values() if kind == "chain"]
        assert winners and min(winners) >= min(slots + 1, 64), (name, winners)
    # what still never fills: the 4-wave wide lists of 10 .. 32 slots (one query block, 16 tiles per stream, 8 per parity list)
    for name in fc.CASES:
        if fc.family(name) == "scan_wide" and name not in fc.MULTI_BLOCK:
            r = plans[(name,) + fc.CASES[name][0:4:3]]
            assert r["n_tiles"] // r["streams"] == 16 and fc.template_args(name)[1] == 4


def test_the_ticket_rule_is_the_planners(exe, cus, plans):
    """takes_ticket decides on the device which launches are repeated under TICKET_ENV: it is finish_plan's rule, on every shape."""
    n_ticket = collections.Counter()
    for leg, env in fc.LEGS.items():
        todo = [(name, nq, n) for name in fc.CASES for nq, n, l, _ in shapes_of(name) if l == leg]
        cases = [(nq, fc.CASES[name][1], fc.CASES[name][2], n, fc.CASES[name][4]) for name, nq, n in todo]
        for (name, nq, n), r in zip(todo, plan(exe, cus, cases, dict(env, **fc.TICKET_ENV))):
            assert r["name"] == name
            assert bool(r["ticket"]) == bool(fc.takes_ticket(name, n, r["streams"], r["qblocks"])), (name, nq, n, r)
            if r["ticket"]:
                assert r["nt"] == 1 and 2 * r["streams"] <= r["t_dyn"] < r["n_tiles"]
                n_ticket[fc.family(name)] += (nq, n) == fc.CASES[name][0:4:3]
    print(dict(n_ticket))
    assert n_ticket == {"scan_tb": 64, "scan_wide": 16, "scan_i8": 15}      # ticketed cases (the second shapes run static only)


def test_planted_rows_never_collide(plans):
    """every corpus the device test builds: the three structures of all planted queries fit side by side"""
    for (name, nq, n), r in plans.items():
        tile_rows, s_, stride = r["tile_rows"], r["streams"], fc.chain_stride(name)
        p = fc.plant_positions(n, tile_rows, s_, nq, stride)
        assert {kind for kind, _ in p.values()} == set(fc.KINDS), name
        for q, (kind, rows) in p.items():
            if kind == "packed":       # 64 rows in a row, starting three rows before a tile boundary
                assert len(rows) == 64 and rows == list(range(rows[0], rows[0] + 64)) and (rows[0] + 3) % tile_rows == 0
            elif kind == "chain":      # one row per tile, tiles of one stream from its first, every visit or every second
                t = [x // tile_rows for x in rows]
                assert t[0] < s_ and all(b - a == stride * s_ for a, b in zip(t, t[1:]))
                assert len(rows) == min(64, len(range(t[0], n // tile_rows, stride * s_)))
            else:
                assert len(rows) == 6 and rows[0] < 3 and rows[-1] >= n - 3 and rows[2] == rows[1] + 1


def test_planted_rows_fit_the_grid_of_staging_variant_1(exe, cus):
    """CRS_SCAN_VARIANT=1 keeps one workgroup per CU: half the streams, 64 for the shape above the bootstrap"""
    names = [n for n in fc.CASES if fc.family(n) == "scan_f16"]
    todo = [(name, nq, n) for name in names for nq, n, _, _ in shapes_of(name)]
    cases = [(nq, fc.CASES[name][1], fc.CASES[name][2], n, F16) for name, nq, n in todo]
    rows = plan(exe, cus, cases, dict(fc.LEGS["CRS_SCAN_TB=0"], CRS_SCAN_VARIANT="1"))
    assert min(r["streams"] for r in rows) == 64
    for (name, nq, n), r in zip(todo, rows):
        assert r["name"] == name
        assert len(fc.plant_positions(n, r["tile_rows"], r["streams"], nq)) >= 6


def corpus(plans, name):
    nq, n = fc.CASES[name][0:4:3]
    return fc.corpus_of(name, nq, n, plans[(name, nq, n)]["streams"])


@pytest.mark.parametrize("name", ["scan_tb_kernel<128,32,4,0>", "scan_i8_kernel<256,32,16,0>", "scan_tb_kernel<640,16,4,0>"])
def test_the_reference_alone_separates_what_was_planted(plans, name):
    """One fp16 corpus, one int8 corpus, one with 16-row tiles: in fp64, after rounding to the slab's format, planted winners
    are >= 10 x BAND from each other and from every other row, duplicates are bit-equal, and every |score| <= 1 -- which is what
    lets the device test ask for exact id lists on the planted queries with check_topk's own band.  (build_corpus asserts the
    same on every corpus it builds.)"""
    assert (fc.CASES[name][4], fc.tile_rows_of(name)) in ((F16, 32), (I8, 32), (F16, 16))
    c = corpus(plans, name)
    fc.check_reference(c, BAND)
    nq, n = c.full64.shape
    assert (nq, n) == (fc.CASES[name][0], fc.CASES[name][3]) and len(c.planted) >= 6
    for q, (kind, rows) in c.planted.items():
        top = np.lexsort((np.arange(n), -c.full64[q]))[:len(rows)]
        assert np.array_equal(top, fc.expected_prefix(c, q, len(rows))), (q, kind)      # they lead the fp64 order, ties by id
        if kind == "duplicates":
            assert np.array_equal(top, np.sort(top))


def test_the_device_check_rejects_wrong_lists(plans):
    """check_lists, the check every device run goes through, on a stand-in for the device: the fp64 top-k rounded to fp32
    passes; a list that misses a planted winner, holds the (k + 1)-th row, orders two duplicates by descending id, drops the
    duplicate of the ragged last tile, or is 3e-5 off in one score does not."""
    name = "scan_tb_kernel<128,32,4,0>"
    c, k = corpus(plans, name), 10
    nq, n = c.full64.shape
    ids = np.stack([np.lexsort((np.arange(n), -c.full64[q]))[:k + 1] for q in range(nq)]).astype(np.int64)
    sc = np.take_along_axis(c.full64, ids, 1).astype(np.float32)
    fc.check_lists(name, c, sc[:, :k], ids[:, :k], k)
    by_kind = {kind: q for q, (kind, rows) in reversed(list(c.planted.items()))}

    def broken(change):
        s, i = sc[:, :k].copy(), ids[:, :k].copy()
        change(s, i)
        with pytest.raises(AssertionError):
            fc.check_lists(name, c, s, i, k)

    def lose_a_winner(s, i):        # the chain's best tile never reached the list: everything moves up, the 11th row comes in
        q = by_kind["packed"]
        s[q], i[q] = sc[q, 1:], ids[q, 1:]

    def next_best_row(s, i):        # a random query returns the (k + 1)-th row in place of the k-th
        q = next(q for q in range(nq) if q not in c.planted and c.full64[q, ids[q, k - 1]] - c.full64[q, ids[q, k]] > 2 * BAND)
        s[q, k - 1], i[q, k - 1] = sc[q, k], ids[q, k]

    def duplicates_descending(s, i):
        q = by_kind["duplicates"]
        i[q, [0, 1]] = i[q, [1, 0]]

    def last_tile_duplicate_lost(s, i):
        q = by_kind["duplicates"]
        assert i[q, 5] >= n - 3
        s[q, 5:], i[q, 5:] = sc[q, 6:], ids[q, 6:]

    def score_off(s, i):
        s[3, 4] += np.float32(3e-5)

    for change in (lose_a_winner, next_best_row, duplicates_descending, last_tile_duplicate_lost, score_off):
        broken(change)


def test_the_cases_take_every_regime_of_the_stage_2_merge(plans):
    """merge.hip picks by (queries, lists, entries per list): one pass at 32 candidates per thread (<= 8192), one pass at 64
    (<= 16384, few queries), or two levels.  merge_slice_cand / merge_slices_for are restated in _scan_form_cases.merge_regime."""
    assert fc.merge_regime(64, 512, 16) == "32 per thread" and fc.merge_regime(64, 512, 32) == "64 per thread"
    assert fc.merge_regime(128, 512, 32) == "two-level" and fc.merge_regime(64, 512, 33) == "two-level"
    seen = collections.Counter(fc.merge_regime(nq, r["streams"], r["kp"]) for (name, nq, n), r in plans.items())
    print(dict(seen))
    assert set(seen) == {"32 per thread", "64 per thread", "two-level"}


# What the GPU suite launched before this table existed: the shapes of tests/test_scan_gpu.py, test_scan_wide_gpu.py (both again
# under CRS_SCAN_TB=0 CRS_SCAN_WIDE=0: test_scan_classic_gpu.py), test_scan_i8_gpu.py, test_scan_dynamic_gpu.py, test_plan_gpu.py
# and test_sweep_group_gpu.py, as (nq, dim, k, n_rows, slab_type).
_NARROW = [(8, 384, 10, 4096), (64, 768, 10, 5000), (1, 384, 3, 1000), (70, 384, 6, 3001), (16, 128, 1, 2048), (33, 384, 16, 2500),
           (20, 384, 17, 2500), (64, 384, 40, 6000), (5, 768, 64, 3000), (9, 100, 5, 777), (3, 1024, 10, 100), (64, 256, 10, 20000),
           (4, 384, 10, 1), (4, 384, 10, 5), (4, 384, 16, 16), (4, 384, 40, 33), (3, 384, 10, 3000), (3, 384, 40, 3000),
           (8, 384, 10, 4096), (16, 384, 10, 6000), (16, 384, 33, 6000), (4, 384, 7, 3000), (64, 384, 10, 100_000),
           (64, 384, 20, 300_000), (7, 384, 32, 300_000), (64, 128, 17, 300_000), (33, 384, 40, 300_000), (64, 256, 64, 300_000),
           (64, 768, 40, 160_000), (64, 384, 56, 300_000), (64, 512, 48, 500_000)]
_NARROW_I8 = [(64, 768, 32, 300_000), (64, 768, 40, 300_000)]
_WIDE = [(65, 384, 10, 3001), (128, 384, 10, 5000), (129, 384, 6, 5000), (256, 384, 10, 20000), (300, 384, 10, 9000),
         (512, 384, 16, 4000), (200, 128, 1, 2500), (100, 256, 16, 2500), (160, 512, 10, 3000), (90, 100, 5, 777), (256, 384, 10, 40),
         (130, 384, 10, 1), (130, 384, 10, 5), (130, 384, 16, 16), (130, 384, 12, 31), (140, 384, 10, 3000), (140, 384, 16, 3000),
         (256, 384, 10, 4096), (200, 384, 10, 6000), (200, 384, 16, 6000), (256, 384, 10, 30000), (64, 384, 10, 30000),
         (8, 384, 10, 5000), (200, 384, 10, 5000), (16, 768, 16, 3000), (16, 768, 5, 3000), (40, 1024, 16, 3000), (40, 1024, 5, 3000),
         (64, 384, 16, 3000), (64, 384, 5, 3000), (130, 256, 16, 3000), (130, 256, 5, 3000), (130, 768, 10, 3000),
         (100, 1024, 16, 2000), (70, 640, 6, 2500), (200, 896, 3, 1800), (64, 768, 10, 150_000), (64, 384, 10, 400_000),
         (64, 384, 16, 400_000), (32, 128, 4, 300_000), (8, 384, 10, 400_000), (256, 768, 10, 2_200_000), (256, 768, 10, 1_000_000)]
_I8 = [(8, 768, 10, 4096), (64, 768, 10, 5001), (33, 384, 6, 3000), (1, 256, 3, 2000), (20, 768, 17, 2500), (5, 1024, 40, 3000),
       (9, 100, 5, 777), (3, 768, 10, 7), (4, 768, 10, 3000), (64, 768, 10, 400_000), (16, 256, 4, 300_000), (130, 768, 16, 60_000),
       (64, 512, 10, 20_000), (64, 256, 1, 20_000), (40, 768, 3, 70_000), (4, 768, 10, 400_000),
       (64, 768, 16, 300_000), (17, 768, 10, 300_001), (64, 384, 32, 250_000), (64, 768, 10, 4096), (64, 768, 10, 300_000)]
_DYNAMIC = [(64, 384, 10, 400_000), (64, 384, 24, 400_001), (7, 384, 10, 300_000), (64, 384, 16, 300_000), (64, 768, 10, 250_000),
            (64, 128, 10, 600_000), (33, 256, 32, 350_000)]
_PLAN = [(64, 384, 10, 4096), (64, 128, 16, 300_000), (64, 128, 24, 300_000), (64, 512, 64, 300_000), (128, 384, 16, 20_000),
         (256, 384, 16, 20_000), (256, 384, 24, 20_000), (256, 768, 16, 20_000)]
_SWEEP = [(nq, d, kc, n) for d, n in ((128, 600_011), (256, 600_011), (384, 1_000_003)) for nq in (64, 65, 128, 192, 256)
          for kc in (16, 24, 32)]


def test_forms_the_suite_reached_before_this_table(exe, cus):
    """The same planner over the shapes the other scan tests launch: how many of the forms they run.  Printed for the record
    (DESIGN.md section 3.1); the assertion only says that the table was needed."""
    f16 = [c + (F16,) for c in _NARROW + _WIDE + _DYNAMIC + _PLAN + _SWEEP]
    i8 = [c + (I8,) for c in _NARROW_I8 + _I8]
    reached = {r["name"] for r in plan(exe, cus, f16 + i8, {})}
    reached |= {r["name"] for r in plan(exe, cus, [c + (F16,) for c in _NARROW + _WIDE], {"CRS_SCAN_TB": "0", "CRS_SCAN_WIDE": "0"})}
    assert reached <= set(fc.CASES)
    fam = collections.Counter(fc.family(n) for n in reached)
    print("forms launched by the suite before tests/test_scan_forms_gpu.py: %d of %d %s" % (len(reached), len(fc.CASES), dict(fam)))
    assert 40 <= len(reached) < 100
