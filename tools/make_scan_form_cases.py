#!/usr/bin/env python3
"""Prints the tables of tests/_scan_form_cases.py (CASES, BOOT_ABOVE, MULTI_BLOCK, LONG_STREAM): shapes for every scan kernel
instantiation, found by a search over the stand-alone planner.  No HIP, no device.

    g++ -O2 -std=c++17 -o plan_table tools/plan_table.cpp compressed-rag-suite_amd/csrc/plan.cpp
    python tools/make_scan_form_cases.py ./plan_table        # paste over the tables when scan_forms.h or plan.cpp changes

tests/test_scan_forms_cpu.py imports generate() and holds the committed tables to it.  The rules (256 CUs):
  * a form takes the first leg, in LEGS' order, whose knobs reach it; the threshold forms take CRS_SCAN_TB=0 (only there does
    their smallest k select the same form as their largest);
  * shard sizes come from LADDER (64 m + 37 rows: ragged for 16-, 32- and 64-row tiles); chain forms take the smallest rung that
    selects them at their largest k with one query block; dump forms the largest rung up to DUMP_MAX at which k = 1 dumps too;
    threshold forms DUMP_MAX with at most 64 queries; wide forms WIDE_N;
  * the query count is the first of NQS that gives such a shape; k is the largest k of the shape that selects the form;
  * LONG_STREAM: a scan_tb / scan_i8 chain form whose case gives a workgroup fewer than slots + 2 tiles runs a second time on the
    smallest rung -- then the first leg, then the first query count of NQS -- at which every workgroup sees more tiles
    than the chain has slots (several query blocks share the CUs, so there are fewer streams; the last rung, 435 237 rows, is
    there for scan_tb_kernel<128,32,4,16>: 64 queries at most, 768 streams)."""
import collections
import os
import subprocess
import sys

COLS = ("family waves slots tile_rows n_tiles streams qblocks kp nt ticket t_dyn dyn_mask boot sched no_stagger mfma form_exists "
        "workspace_bytes text").split()
LEGS = [("default", {}), ("CRS_SCAN_TB=0", {"CRS_SCAN_TB": "0"}), ("CRS_SCAN_WIDE=0", {"CRS_SCAN_WIDE": "0"}),
        ("CRS_SCAN_W1=0", {"CRS_SCAN_W1": "0"}), ("CRS_WIDE_MFMA=16", {"CRS_WIDE_MFMA": "16"}), ("CRS_WIDE_MFMA=32", {"CRS_WIDE_MFMA": "32"})]
LADDER = [64 * m + 37 for m in (32, 64, 128, 256, 512, 1024, 1536, 2048, 2560, 3072, 3584, 4096, 4112, 4688, 6800)]
NQS = [61, 37, 100, 200]
DUMP_MAX = 64 * 1024 + 37
WIDE_N = 64 * 4096 + 37
BOOT_SHAPE = (200, 64 * 2048 + 37)      # four query blocks: 32 rounds, above the bootstrap's 24
MULTI_NQ = 300                          # two query blocks of the 8-wave wide forms
CUS = 256


def plan(exe, cases, env, cus=CUS):
    """cases: (nq, dim, k, n_rows, slab_type) -> one dict per case; "name" is spelled as `plan_table --forms` spells it"""
    e = {k: v for k, v in os.environ.items() if not k.startswith("CRS_")}
    e.update(env)
    out = subprocess.run([exe, str(cus)], input="".join("%d %d %d %d %d\n" % c for c in cases), env=e, capture_output=True, text=True,
                         check=True, timeout=300).stdout.splitlines()
    assert len(out) == len(cases)
    rows = [{n: (v if n in ("family", "text") else int(v)) for n, v in zip(COLS, line.split("\t"))} for line in out]
    for r in rows:
        r["name"] = r["text"].split(" ")[0] + ("/mfma%d" % r["mfma"] if r["family"] == "Wide" else "")
    return rows


def list_forms(exe):
    return subprocess.run([exe, "--forms"], capture_output=True, text=True, check=True, timeout=60).stdout.split()


def generate(exe):
    """-> {"CASES": {form: (nq, dim, k, n_rows, slab_type, leg)}, "BOOT_ABOVE" / "MULTI_BLOCK": {form: (nq, n_rows)},
    "LONG_STREAM": {form: (nq, n_rows, leg)}}"""
    forms = list_forms(exe)
    grid = [(nq, pdim, k, n, st) for st, pdims in ((0, range(128, 1025, 128)), (1, range(256, 1025, 256))) for pdim in pdims
            for nq in NQS for k in range(1, 65) for n in LADDER]
    reach = {}      # leg -> form -> [(case, plan)]
    for leg, env in LEGS:
        reach[leg] = collections.defaultdict(list)
        for c, r in zip(grid, plan(exe, grid, env)):
            reach[leg][r["name"]].append((c, r))

    cases, boot_above, multi_block, long_stream = {}, {}, {}, {}
    for f in forms:
        args = [int(x) for x in f.split("/")[0].split("<")[1].rstrip(">").split(",")]
        classic = f.startswith("scan_f16") or f.endswith(",-1>")
        dump = f.startswith("scan_w2") or (f.startswith(("scan_tb", "scan_i8")) and args[-1] == 0)
        wide = f.startswith("scan_wide")
        leg = "CRS_SCAN_TB=0" if classic else next(l for l, _ in LEGS if f in reach[l])
        env = dict(LEGS)[leg]
        plans = {(c[0], c[3], c[2]): r for c, r in reach[leg][f]}
        ks = collections.defaultdict(set)       # (nq, n_rows) -> the k that select the form
        for nq, n, k in plans:
            ks[(nq, n)].add(k)
        kmax = max(k for _, _, k in plans)
        if classic:
            kmin = 1 if args[2] == 16 else 17
            shapes = [s for s, have in ks.items() if s[1] == DUMP_MAX and s[0] <= 64 and kmin in have and kmax in have]
        elif dump:
            shapes = [s for s, have in ks.items() if s[1] <= DUMP_MAX and 1 in have and kmax in have]
            shapes = [s for s in shapes if s[1] == max(n for _, n in shapes)]
        elif wide:
            shapes = [s for s, have in ks.items() if s[1] == WIDE_N and kmax in have]
        else:
            shapes = [s for s, have in ks.items() if kmax in have]
            shapes = [s for s in shapes if plans[s + (kmax,)]["qblocks"] == 1] or shapes
            shapes = [s for s in shapes if s[1] == min(n for _, n in shapes)]
        nq, n = min(shapes, key=lambda s: (plans[s + (kmax,)]["qblocks"], NQS.index(s[0])))
        r = plans[(nq, n, kmax)]
        st = 1 if f.startswith("scan_i8") else 0
        cases[f] = (nq, args[0], kmax, n, st, leg)
        if wide and args[1] == 8:
            m, = plan(exe, [(MULTI_NQ, args[0], kmax, WIDE_N, 0)], env)
            assert m["name"] == f and m["qblocks"] == 2 and m["n_tiles"] // m["streams"] >= 32, m
            multi_block[f] = (MULTI_NQ, WIDE_N)
        if f.startswith("scan_f16") and args[1:] == [32, 16]:
            b, = plan(exe, [(BOOT_SHAPE[0], args[0], kmax, BOOT_SHAPE[1], 0)], env)
            assert r["boot"] == 1 and b["name"] == f and b["boot"] == 0, b
            boot_above[f] = BOOT_SHAPE
        slots = args[-1]
        if f.startswith(("scan_tb", "scan_i8")) and slots > 0 and r["n_tiles"] // r["streams"] < slots + 2:
            found = [(c[3], LEGS.index((l, e)), NQS.index(c[0]), c[0], l) for l, e in LEGS for c, p in reach[l].get(f, [])
                     if c[2] == kmax and p["n_tiles"] // p["streams"] > slots]
            assert found, (f, r["n_tiles"], r["streams"])
            n2, _, _, nq2, leg2 = min(found)
            long_stream[f] = (nq2, n2, leg2)

    return {"CASES": cases, "BOOT_ABOVE": boot_above, "MULTI_BLOCK": multi_block, "LONG_STREAM": long_stream}


def main(exe):
    t = generate(exe)
    out = ["CASES = {"]
    out += ['    "%s": (%d, %d, %d, %d, %s, "%s"),' % ((f,) + c[:4] + ("I8" if c[4] else "F16", c[5])) for f, c in t["CASES"].items()]
    for title in ("BOOT_ABOVE", "MULTI_BLOCK"):
        out += ["}", "", title + " = {"] + ['    "%s": (%d, %d),' % ((f,) + v) for f, v in t[title].items()]
    out += ["}", "", "LONG_STREAM = {"] + ['    "%s": (%d, %d, "%s"),' % ((f,) + v) for f, v in t["LONG_STREAM"].items()] + ["}"]
    print("\n".join(out))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_scan_form_cases.py <plan_table binary>")
    main(sys.argv[1])
