"""One search per scan kernel instantiation (tests/test_scan_forms_cpu.py, tests/test_scan_forms_gpu.py).

CASES maps every form name that `plan_table --forms` prints (csrc/scan_forms.h's predicates; wide forms carry /mfma16 or /mfma32)
to (nq, dim, k, n_rows, slab_type, leg): a shape that selects the form at 256 CUs under the leg's knobs.  Second shapes of some
forms: BOOT_ABOVE (nq, n_rows) for the threshold forms that have a bootstrap instantiation (>= 24 rounds: scan.hip's plain form);
MULTI_BLOCK (nq, n_rows) for the 8-wave wide forms (two query blocks, 32 or 64 tiles per stream); LONG_STREAM (nq, n_rows, leg)
for the scan_tb / scan_i8 chain forms whose case gives a workgroup fewer than slots + 2 tiles: a shape, possibly under another
leg, at which every workgroup sees more tiles than the chain has slots.  tools/make_scan_form_cases.py prints the tables from
the rules below and the CPU test holds them to it.  What the planner answers for a shape (streams, query blocks) is read from
the describe text at run time, the tile rows from the form's name; which shapes take the ticketed schedule under
CRS_TB_DYN_MIN=4 CRS_TB_DYN=100 CRS_SCAN_NT=1 is plan.cpp's rule restated (takes_ticket), checked against the planner on the CPU.

How the shapes were chosen (tools/make_scan_form_cases.py: a search over the stand-alone planner, tools/plan_table.cpp):
  * n_rows comes from a ladder of shard sizes 64 m + 37 -- ragged for 16-, 32- and 64-row tiles alike, the last tile holds 5 or 37
    rows -- and is the smallest rung that selects the form with one query block (the ticket needs one block);
  * dump forms take the largest rung <= 65 573 rows at which k = 1 dumps too: several tiles per stream, and streams of unequal
    length, so the dump's slot index and its padding of the shorter streams both run;
  * wide forms exist at any shard size; they take 262 181 rows with one query block (16 tiles per stream, 8 per parity list: the
    4-slot lists fill and displace), and the 8-wave forms run again with 300 queries -- two blocks share the CUs, 32 tiles per
    stream on 64-row tiles, 64 on 32-row tiles: parity lists of up to 16 slots and the split list of 24 fill and displace, the
    split list of 32 fills exactly on 64-row tiles.  The 4-wave forms of 10 .. 32 slots never fill;
  * the threshold forms (scan_f16_kernel, scan_i8_kernel<..,-1>) all run under CRS_SCAN_TB=0: only there does their smallest k
    (1 for 16-slot lists, 17 for 32-slot lists) select the same form as their largest;
  * k is the largest k that selects the form; nq is never a multiple of 16.
With the smallest shard a chain form's workgroup sees 9 to 17 tiles (8193 tiles and more over 512 or 768 streams): the 4-slot
chains, and the 10-slot chains but <128,32,4,10>, fill and displace there; the 45 others are the LONG_STREAM forms, which at
their second shape see slots + 1 tiles at least -- 200 queries are four blocks, 128 streams, 64 tiles of 32 rows or 128 of 16 on
262 181 rows; the 4-wave forms of <= 16 slots on rows that have an 8-wave form exist for <= 64 queries only and take a longer
shard instead (300 069 rows; 435 237 for <128,32,4,16>, the one shape above 300 000 rows).

Corpus (build_corpus): seeded unit rows and queries of norm 0.995, rounded to the slab's format before the fp64 product is taken
(int8: oracle/scan_ref.py's row quantisation and the kernel's 16-bit fixed-point query).  The queries at {0, 15, 16, 31, 32, 63,
64, nq - 1} -- the edges of MFMA column blocks, waves and query blocks -- each get one planted structure, in rotation:
  packed      64 consecutive rows from three rows before a tile boundary, c_j v with c_j ascending in the row number
  chain       one row in each of the tiles s, s + d S, s + 2 d S, ... (S streams), c_j v ascending in that order, 64 at most
  duplicates  the query itself as a row at six places: a row, its neighbour, the first row of the next tile, a tile of another
              workgroup, one of the shard's first rows and one of the ragged last tile's
with v the query and c_j = 0.95 - 0.004 (63 - j): 0.698 .. 0.95, above any random row (the best of 262 k random unit rows of 128
elements scores about 0.45) and 0.004 apart, a hundred times 10 x BAND, which also covers int8 rounding (about 4e-4 per score).

Tile -> workgroup -> list (scan_common.h's grid mapping; scan_tb.hip, scan_i8.hip, scan_wide.hip "Tile order"): under the static
schedule workgroup `stream` of a query block walks tiles stream, stream + S, stream + 2 S, ...  scan_tb / scan_i8 chain forms
keep ONE list per (query, workgroup) -- the query's four lanes insert every tile and hold copies: d = 1, the winners are ALL
tiles of workgroup s from its first.  scan_wide forms of <= 16 slots keep two lists per (query, workgroup), one per lane of the
pair: lane half h takes the tiles of the workgroup's iterations of parity h; the 24- / 32-slot forms keep one list split across
the pair: d = 2, the even iterations of workgroup s, one list in either kind.  Each winner is better than all before it, so it
goes to the head and shifts the whole list down; once the stream has more tiles than the list has slots the tail falls off.
A stream with fewer than 64 d tiles gets as many winners as it has such tiles.
"""
import collections
import functools
import os
import sys

import numpy as np

F16, I8 = 0, 1
LEGS = collections.OrderedDict([
    ("default", {}), ("CRS_SCAN_TB=0", {"CRS_SCAN_TB": "0"}), ("CRS_SCAN_WIDE=0", {"CRS_SCAN_WIDE": "0"}),
    ("CRS_SCAN_W1=0", {"CRS_SCAN_W1": "0"}), ("CRS_WIDE_MFMA=16", {"CRS_WIDE_MFMA": "16"}), ("CRS_WIDE_MFMA=32", {"CRS_WIDE_MFMA": "32"})])
CHILD_LEGS = ("CRS_SCAN_TB=0", "CRS_SCAN_WIDE=0", "CRS_SCAN_W1=0")    # knobs a process reads once
TICKET_ENV = {"CRS_TB_DYN_MIN": "4", "CRS_TB_DYN": "100", "CRS_SCAN_NT": "1"}   # re-read per call
ID_BASE = (1 << 40) + 5
POISON = 0xAB
CUS = 256

CASES = {
    "scan_tb_kernel<128,32,4,0>": (61, 128, 64, 65573, F16, "default"),
    "scan_tb_kernel<128,32,4,4>": (61, 128, 4, 196645, F16, "default"),
    "scan_tb_kernel<128,32,4,10>": (61, 128, 10, 262181, F16, "default"),
    "scan_tb_kernel<128,32,4,16>": (61, 128, 16, 262181, F16, "default"),
    "scan_tb_kernel<128,32,4,24>": (61, 128, 24, 262181, F16, "default"),
    "scan_tb_kernel<128,32,4,32>": (61, 128, 32, 262181, F16, "default"),
    "scan_tb_kernel<128,32,8,0>": (100, 128, 16, 65573, F16, "CRS_SCAN_WIDE=0"),
    "scan_tb_kernel<128,32,8,4>": (100, 128, 4, 131109, F16, "CRS_SCAN_WIDE=0"),
    "scan_tb_kernel<128,32,8,10>": (100, 128, 10, 262181, F16, "CRS_SCAN_WIDE=0"),
    "scan_tb_kernel<128,32,8,16>": (100, 128, 16, 262181, F16, "CRS_SCAN_WIDE=0"),
    "scan_wide_kernel<128,4,4>/mfma32": (100, 128, 4, 262181, F16, "default"),
    "scan_wide_kernel<128,4,10>/mfma32": (100, 128, 10, 262181, F16, "default"),
    "scan_wide_kernel<128,4,16>/mfma32": (100, 128, 16, 262181, F16, "default"),
    "scan_wide_kernel<128,4,24>/mfma32": (100, 128, 24, 262181, F16, "default"),
    "scan_wide_kernel<128,4,32>/mfma32": (100, 128, 32, 262181, F16, "default"),
    "scan_wide_kernel<128,8,4>/mfma32": (200, 128, 4, 262181, F16, "default"),
    "scan_wide_kernel<128,8,10>/mfma32": (200, 128, 10, 262181, F16, "default"),
    "scan_wide_kernel<128,8,16>/mfma32": (200, 128, 16, 262181, F16, "default"),
    "scan_wide_kernel<128,8,24>/mfma32": (200, 128, 24, 262181, F16, "default"),
    "scan_wide_kernel<128,8,32>/mfma32": (200, 128, 32, 262181, F16, "default"),
    "scan_f16_kernel<128,32,16>": (61, 128, 16, 65573, F16, "CRS_SCAN_TB=0"),
    "scan_f16_kernel<128,32,32>": (61, 128, 64, 65573, F16, "CRS_SCAN_TB=0"),
    "scan_tb_kernel<256,32,4,0>": (61, 256, 64, 65573, F16, "default"),
    "scan_tb_kernel<256,32,4,4>": (61, 256, 4, 131109, F16, "default"),
    "scan_tb_kernel<256,32,4,10>": (61, 256, 10, 262181, F16, "default"),
    "scan_tb_kernel<256,32,4,16>": (61, 256, 16, 262181, F16, "default"),
    "scan_tb_kernel<256,32,4,24>": (61, 256, 24, 262181, F16, "default"),
    "scan_tb_kernel<256,32,4,32>": (61, 256, 32, 262181, F16, "default"),
    "scan_tb_kernel<256,32,4,64>": (61, 256, 64, 262181, F16, "default"),
    "scan_tb_kernel<256,32,8,0>": (100, 256, 16, 65573, F16, "CRS_SCAN_WIDE=0"),
    "scan_tb_kernel<256,32,8,4>": (100, 256, 4, 131109, F16, "CRS_SCAN_WIDE=0"),
    "scan_tb_kernel<256,32,8,10>": (100, 256, 10, 262181, F16, "CRS_SCAN_WIDE=0"),
    "scan_tb_kernel<256,32,8,16>": (100, 256, 16, 262181, F16, "CRS_SCAN_WIDE=0"),
    "scan_wide_kernel<256,4,4>/mfma32": (100, 256, 4, 262181, F16, "default"),
    "scan_wide_kernel<256,4,10>/mfma32": (100, 256, 10, 262181, F16, "default"),
    "scan_wide_kernel<256,4,16>/mfma32": (100, 256, 16, 262181, F16, "default"),
    "scan_wide_kernel<256,4,24>/mfma32": (100, 256, 24, 262181, F16, "default"),
    "scan_wide_kernel<256,4,32>/mfma32": (100, 256, 32, 262181, F16, "default"),
    "scan_wide_kernel<256,8,4>/mfma32": (200, 256, 4, 262181, F16, "default"),
    "scan_wide_kernel<256,8,10>/mfma32": (200, 256, 10, 262181, F16, "default"),
    "scan_wide_kernel<256,8,16>/mfma32": (200, 256, 16, 262181, F16, "default"),
    "scan_wide_kernel<256,8,24>/mfma16": (200, 256, 24, 262181, F16, "CRS_WIDE_MFMA=16"),
    "scan_wide_kernel<256,8,24>/mfma32": (200, 256, 24, 262181, F16, "default"),
    "scan_wide_kernel<256,8,32>/mfma16": (200, 256, 32, 262181, F16, "CRS_WIDE_MFMA=16"),
    "scan_wide_kernel<256,8,32>/mfma32": (200, 256, 32, 262181, F16, "default"),
    "scan_i8_kernel<256,32,16,0>": (61, 256, 64, 65573, I8, "default"),
    "scan_i8_kernel<256,32,16,4>": (61, 256, 4, 131109, I8, "default"),
    "scan_i8_kernel<256,32,16,10>": (61, 256, 10, 262181, I8, "default"),
    "scan_i8_kernel<256,32,16,16>": (61, 256, 16, 262181, I8, "default"),
    "scan_i8_kernel<256,32,16,32>": (61, 256, 32, 262181, I8, "default"),
    "scan_i8_kernel<256,32,16,48>": (61, 256, 48, 262181, I8, "default"),
    "scan_i8_kernel<256,32,16,-1>": (61, 256, 16, 65573, I8, "CRS_SCAN_TB=0"),
    "scan_f16_kernel<256,32,16>": (61, 256, 16, 65573, F16, "CRS_SCAN_TB=0"),
    "scan_i8_kernel<256,32,32,-1>": (61, 256, 64, 65573, I8, "CRS_SCAN_TB=0"),
    "scan_f16_kernel<256,32,32>": (61, 256, 64, 65573, F16, "CRS_SCAN_TB=0"),
    "scan_tb_kernel<384,32,4,0>": (61, 384, 64, 65573, F16, "default"),
    "scan_tb_kernel<384,32,4,4>": (61, 384, 4, 131109, F16, "default"),
    "scan_tb_kernel<384,32,4,10>": (61, 384, 10, 262181, F16, "default"),
    "scan_tb_kernel<384,32,4,16>": (61, 384, 16, 262181, F16, "default"),
    "scan_tb_kernel<384,32,4,24>": (61, 384, 24, 262181, F16, "default"),
    "scan_tb_kernel<384,32,4,32>": (61, 384, 32, 262181, F16, "default"),
    "scan_tb_kernel<384,32,4,48>": (61, 384, 48, 262181, F16, "default"),
    "scan_tb_kernel<384,32,4,56>": (61, 384, 56, 262181, F16, "default"),
    "scan_tb_kernel<384,32,8,0>": (100, 384, 16, 65573, F16, "CRS_SCAN_WIDE=0"),
    "scan_tb_kernel<384,32,8,4>": (100, 384, 4, 131109, F16, "CRS_SCAN_WIDE=0"),
    "scan_tb_kernel<384,32,8,10>": (100, 384, 10, 262181, F16, "CRS_SCAN_WIDE=0"),
    "scan_tb_kernel<384,32,8,16>": (100, 384, 16, 262181, F16, "CRS_SCAN_WIDE=0"),
    "scan_wide_kernel<384,4,4>/mfma32": (100, 384, 4, 262181, F16, "default"),
    "scan_wide_kernel<384,4,10>/mfma32": (100, 384, 10, 262181, F16, "default"),
    "scan_wide_kernel<384,4,16>/mfma32": (100, 384, 16, 262181, F16, "default"),
    "scan_wide_kernel<384,4,24>/mfma32": (100, 384, 24, 262181, F16, "default"),
    "scan_wide_kernel<384,4,32>/mfma32": (100, 384, 32, 262181, F16, "default"),
    "scan_wide_kernel<384,8,4>/mfma32": (200, 384, 4, 262181, F16, "default"),
    "scan_wide_kernel<384,8,10>/mfma32": (200, 384, 10, 262181, F16, "default"),
    "scan_wide_kernel<384,8,16>/mfma32": (200, 384, 16, 262181, F16, "default"),
    "scan_wide_kernel<384,8,24>/mfma16": (200, 384, 24, 262181, F16, "default"),
    "scan_wide_kernel<384,8,24>/mfma32": (200, 384, 24, 262181, F16, "CRS_WIDE_MFMA=32"),
    "scan_wide_kernel<384,8,32>/mfma16": (200, 384, 32, 262181, F16, "default"),
    "scan_wide_kernel<384,8,32>/mfma32": (200, 384, 32, 262181, F16, "CRS_WIDE_MFMA=32"),
    "scan_f16_kernel<384,32,16>": (61, 384, 16, 65573, F16, "CRS_SCAN_TB=0"),
    "scan_f16_kernel<384,32,32>": (61, 384, 64, 65573, F16, "CRS_SCAN_TB=0"),
    "scan_tb_kernel<512,32,4,0>": (61, 512, 64, 65573, F16, "default"),
    "scan_tb_kernel<512,32,4,4>": (61, 512, 4, 131109, F16, "default"),
    "scan_tb_kernel<512,32,4,10>": (61, 512, 10, 262181, F16, "default"),
    "scan_tb_kernel<512,32,4,16>": (61, 512, 16, 262181, F16, "default"),
    "scan_tb_kernel<512,32,4,24>": (61, 512, 24, 262181, F16, "default"),
    "scan_tb_kernel<512,32,4,32>": (61, 512, 32, 262181, F16, "default"),
    "scan_tb_kernel<512,32,4,48>": (61, 512, 48, 262181, F16, "default"),
    "scan_tb_kernel<512,32,8,0>": (100, 512, 16, 32805, F16, "CRS_SCAN_WIDE=0"),
    "scan_tb_kernel<512,32,8,4>": (100, 512, 4, 65573, F16, "CRS_SCAN_WIDE=0"),
    "scan_tb_kernel<512,32,8,10>": (100, 512, 10, 163877, F16, "CRS_SCAN_WIDE=0"),
    "scan_tb_kernel<512,32,8,16>": (100, 512, 16, 262181, F16, "CRS_SCAN_WIDE=0"),
    "scan_wide_kernel<512,4,4>/mfma32": (100, 512, 4, 262181, F16, "default"),
    "scan_wide_kernel<512,4,10>/mfma32": (100, 512, 10, 262181, F16, "default"),
    "scan_wide_kernel<512,4,16>/mfma32": (100, 512, 16, 262181, F16, "default"),
    "scan_wide_kernel<512,8,4>/mfma32": (200, 512, 4, 262181, F16, "default"),
    "scan_wide_kernel<512,8,10>/mfma32": (200, 512, 10, 262181, F16, "default"),
    "scan_wide_kernel<512,8,16>/mfma32": (200, 512, 16, 262181, F16, "default"),
    "scan_i8_kernel<512,32,16,0>": (61, 512, 64, 65573, I8, "default"),
    "scan_i8_kernel<512,32,16,4>": (61, 512, 4, 131109, I8, "default"),
    "scan_i8_kernel<512,32,16,10>": (61, 512, 10, 262181, I8, "default"),
    "scan_i8_kernel<512,32,16,16>": (61, 512, 16, 262181, I8, "default"),
    "scan_i8_kernel<512,32,16,32>": (61, 512, 32, 262181, I8, "default"),
    "scan_i8_kernel<512,32,16,48>": (61, 512, 48, 262181, I8, "default"),
    "scan_i8_kernel<512,32,16,-1>": (61, 512, 16, 65573, I8, "CRS_SCAN_TB=0"),
    "scan_f16_kernel<512,32,16>": (61, 512, 16, 65573, F16, "CRS_SCAN_TB=0"),
    "scan_i8_kernel<512,32,32,-1>": (61, 512, 64, 65573, I8, "CRS_SCAN_TB=0"),
    "scan_f16_kernel<512,32,32>": (61, 512, 64, 65573, F16, "CRS_SCAN_TB=0"),
    "scan_tb_kernel<640,16,4,0>": (61, 640, 64, 32805, F16, "default"),
    "scan_tb_kernel<640,16,4,4>": (61, 640, 4, 65573, F16, "default"),
    "scan_tb_kernel<640,16,4,10>": (61, 640, 10, 131109, F16, "default"),
    "scan_tb_kernel<640,16,4,16>": (61, 640, 16, 131109, F16, "default"),
    "scan_tb_kernel<640,16,4,24>": (61, 640, 24, 131109, F16, "default"),
    "scan_tb_kernel<640,16,4,32>": (61, 640, 32, 131109, F16, "default"),
    "scan_tb_kernel<640,16,4,48>": (61, 640, 48, 131109, F16, "default"),
    "scan_f16_kernel<640,16,16>": (61, 640, 16, 65573, F16, "CRS_SCAN_TB=0"),
    "scan_f16_kernel<640,16,32>": (61, 640, 64, 65573, F16, "CRS_SCAN_TB=0"),
    "scan_tb_kernel<768,16,4,0>": (61, 768, 64, 32805, F16, "default"),
    "scan_tb_kernel<768,16,4,4>": (61, 768, 4, 65573, F16, "default"),
    "scan_tb_kernel<768,16,4,10>": (61, 768, 10, 131109, F16, "default"),
    "scan_tb_kernel<768,16,4,16>": (61, 768, 16, 131109, F16, "default"),
    "scan_tb_kernel<768,16,4,24>": (61, 768, 24, 131109, F16, "default"),
    "scan_tb_kernel<768,16,4,32>": (61, 768, 32, 131109, F16, "default"),
    "scan_tb_kernel<768,16,4,40>": (61, 768, 40, 131109, F16, "default"),
    "scan_tb_kernel<768,16,8,0>": (100, 768, 16, 16421, F16, "CRS_SCAN_W1=0"),
    "scan_tb_kernel<768,16,8,4>": (100, 768, 4, 32805, F16, "CRS_SCAN_W1=0"),
    "scan_tb_kernel<768,16,8,10>": (100, 768, 10, 98341, F16, "CRS_SCAN_W1=0"),
    "scan_tb_kernel<768,16,8,16>": (100, 768, 16, 131109, F16, "CRS_SCAN_W1=0"),
    "scan_i8_kernel<768,32,16,0>": (61, 768, 64, 65573, I8, "default"),
    "scan_i8_kernel<768,32,16,4>": (61, 768, 4, 131109, I8, "default"),
    "scan_i8_kernel<768,32,16,10>": (61, 768, 10, 262181, I8, "default"),
    "scan_i8_kernel<768,32,16,16>": (61, 768, 16, 262181, I8, "default"),
    "scan_i8_kernel<768,32,16,32>": (61, 768, 32, 262181, I8, "default"),
    "scan_i8_kernel<768,32,16,48>": (61, 768, 48, 262181, I8, "default"),
    "scan_i8_kernel<768,32,16,-1>": (61, 768, 16, 65573, I8, "CRS_SCAN_TB=0"),
    "scan_f16_kernel<768,16,16>": (61, 768, 16, 65573, F16, "CRS_SCAN_TB=0"),
    "scan_i8_kernel<768,32,32,-1>": (61, 768, 64, 65573, I8, "CRS_SCAN_TB=0"),
    "scan_f16_kernel<768,16,32>": (61, 768, 64, 65573, F16, "CRS_SCAN_TB=0"),
    "scan_w2_kernel<768>": (100, 768, 64, 65573, F16, "default"),
    "scan_tb_kernel<896,16,4,0>": (61, 896, 64, 32805, F16, "default"),
    "scan_tb_kernel<896,16,4,4>": (61, 896, 4, 65573, F16, "default"),
    "scan_tb_kernel<896,16,4,10>": (61, 896, 10, 131109, F16, "default"),
    "scan_tb_kernel<896,16,4,16>": (61, 896, 16, 131109, F16, "default"),
    "scan_tb_kernel<896,16,4,24>": (61, 896, 24, 131109, F16, "default"),
    "scan_tb_kernel<896,16,4,32>": (61, 896, 32, 131109, F16, "default"),
    "scan_f16_kernel<896,16,16>": (61, 896, 16, 65573, F16, "CRS_SCAN_TB=0"),
    "scan_f16_kernel<896,16,32>": (61, 896, 64, 65573, F16, "CRS_SCAN_TB=0"),
    "scan_tb_kernel<1024,16,4,0>": (61, 1024, 64, 32805, F16, "default"),
    "scan_tb_kernel<1024,16,4,4>": (61, 1024, 4, 65573, F16, "default"),
    "scan_tb_kernel<1024,16,4,10>": (61, 1024, 10, 131109, F16, "default"),
    "scan_tb_kernel<1024,16,4,16>": (61, 1024, 16, 131109, F16, "default"),
    "scan_tb_kernel<1024,16,4,24>": (61, 1024, 24, 131109, F16, "default"),
    "scan_tb_kernel<1024,16,4,32>": (61, 1024, 32, 131109, F16, "default"),
    "scan_tb_kernel<1024,16,8,0>": (100, 1024, 16, 16421, F16, "default"),
    "scan_tb_kernel<1024,16,8,4>": (100, 1024, 4, 32805, F16, "default"),
    "scan_tb_kernel<1024,16,8,10>": (100, 1024, 10, 98341, F16, "default"),
    "scan_tb_kernel<1024,16,8,16>": (100, 1024, 16, 131109, F16, "default"),
    "scan_i8_kernel<1024,32,16,0>": (61, 1024, 64, 65573, I8, "default"),
    "scan_i8_kernel<1024,32,16,4>": (61, 1024, 4, 131109, I8, "default"),
    "scan_i8_kernel<1024,32,16,10>": (61, 1024, 10, 262181, I8, "default"),
    "scan_i8_kernel<1024,32,16,16>": (61, 1024, 16, 262181, I8, "default"),
    "scan_i8_kernel<1024,32,16,32>": (61, 1024, 32, 262181, I8, "default"),
    "scan_i8_kernel<1024,32,16,-1>": (61, 1024, 16, 65573, I8, "CRS_SCAN_TB=0"),
    "scan_f16_kernel<1024,16,16>": (61, 1024, 16, 65573, F16, "CRS_SCAN_TB=0"),
    "scan_i8_kernel<1024,32,32,-1>": (61, 1024, 64, 65573, I8, "CRS_SCAN_TB=0"),
    "scan_f16_kernel<1024,16,32>": (61, 1024, 64, 65573, F16, "CRS_SCAN_TB=0"),
}

BOOT_ABOVE = {
    "scan_f16_kernel<128,32,16>": (200, 131109),
    "scan_f16_kernel<256,32,16>": (200, 131109),
    "scan_f16_kernel<384,32,16>": (200, 131109),
    "scan_f16_kernel<512,32,16>": (200, 131109),
}

MULTI_BLOCK = {
    "scan_wide_kernel<128,8,4>/mfma32": (300, 262181),
    "scan_wide_kernel<128,8,10>/mfma32": (300, 262181),
    "scan_wide_kernel<128,8,16>/mfma32": (300, 262181),
    "scan_wide_kernel<128,8,24>/mfma32": (300, 262181),
    "scan_wide_kernel<128,8,32>/mfma32": (300, 262181),
    "scan_wide_kernel<256,8,4>/mfma32": (300, 262181),
    "scan_wide_kernel<256,8,10>/mfma32": (300, 262181),
    "scan_wide_kernel<256,8,16>/mfma32": (300, 262181),
    "scan_wide_kernel<256,8,24>/mfma16": (300, 262181),
    "scan_wide_kernel<256,8,24>/mfma32": (300, 262181),
    "scan_wide_kernel<256,8,32>/mfma16": (300, 262181),
    "scan_wide_kernel<256,8,32>/mfma32": (300, 262181),
    "scan_wide_kernel<384,8,4>/mfma32": (300, 262181),
    "scan_wide_kernel<384,8,10>/mfma32": (300, 262181),
    "scan_wide_kernel<384,8,16>/mfma32": (300, 262181),
    "scan_wide_kernel<384,8,24>/mfma16": (300, 262181),
    "scan_wide_kernel<384,8,24>/mfma32": (300, 262181),
    "scan_wide_kernel<384,8,32>/mfma16": (300, 262181),
    "scan_wide_kernel<384,8,32>/mfma32": (300, 262181),
    "scan_wide_kernel<512,8,4>/mfma32": (300, 262181),
    "scan_wide_kernel<512,8,10>/mfma32": (300, 262181),
    "scan_wide_kernel<512,8,16>/mfma32": (300, 262181),
}

LONG_STREAM = {
    "scan_tb_kernel<128,32,4,10>": (61, 300069, "default"),
    "scan_tb_kernel<128,32,4,16>": (61, 435237, "default"),
    "scan_tb_kernel<128,32,4,24>": (200, 262181, "CRS_SCAN_WIDE=0"),
    "scan_tb_kernel<128,32,4,32>": (200, 262181, "CRS_SCAN_WIDE=0"),
    "scan_tb_kernel<128,32,8,16>": (200, 262181, "CRS_SCAN_WIDE=0"),
    "scan_tb_kernel<256,32,4,16>": (61, 300069, "default"),
    "scan_tb_kernel<256,32,4,24>": (200, 196645, "CRS_SCAN_WIDE=0"),
    "scan_tb_kernel<256,32,4,32>": (200, 262181, "CRS_SCAN_WIDE=0"),
    "scan_tb_kernel<256,32,4,64>": (200, 300069, "default"),
    "scan_tb_kernel<256,32,8,16>": (200, 262181, "CRS_SCAN_WIDE=0"),
    "scan_i8_kernel<256,32,16,16>": (200, 131109, "default"),
    "scan_i8_kernel<256,32,16,32>": (200, 262181, "default"),
    "scan_i8_kernel<256,32,16,48>": (200, 262181, "default"),
    "scan_tb_kernel<384,32,4,16>": (61, 300069, "default"),
    "scan_tb_kernel<384,32,4,24>": (200, 196645, "CRS_SCAN_WIDE=0"),
    "scan_tb_kernel<384,32,4,32>": (200, 262181, "CRS_SCAN_WIDE=0"),
    "scan_tb_kernel<384,32,4,48>": (200, 262181, "default"),
    "scan_tb_kernel<384,32,4,56>": (200, 262181, "default"),
    "scan_tb_kernel<384,32,8,16>": (200, 262181, "CRS_SCAN_WIDE=0"),
    "scan_tb_kernel<512,32,4,16>": (61, 300069, "default"),
    "scan_tb_kernel<512,32,4,24>": (200, 196645, "default"),
    "scan_tb_kernel<512,32,4,32>": (200, 262181, "default"),
    "scan_tb_kernel<512,32,4,48>": (200, 262181, "default"),
    "scan_i8_kernel<512,32,16,16>": (200, 131109, "default"),
    "scan_i8_kernel<512,32,16,32>": (200, 262181, "default"),
    "scan_i8_kernel<512,32,16,48>": (200, 262181, "default"),
    "scan_tb_kernel<640,16,4,16>": (200, 65573, "default"),
    "scan_tb_kernel<640,16,4,24>": (200, 98341, "default"),
    "scan_tb_kernel<640,16,4,32>": (200, 131109, "default"),
    "scan_tb_kernel<640,16,4,48>": (200, 131109, "default"),
    "scan_tb_kernel<768,16,4,16>": (61, 163877, "default"),
    "scan_tb_kernel<768,16,4,24>": (200, 98341, "CRS_SCAN_W1=0"),
    "scan_tb_kernel<768,16,4,32>": (200, 131109, "CRS_SCAN_W1=0"),
    "scan_tb_kernel<768,16,4,40>": (200, 131109, "CRS_SCAN_W1=0"),
    "scan_i8_kernel<768,32,16,16>": (200, 131109, "default"),
    "scan_i8_kernel<768,32,16,32>": (200, 262181, "default"),
    "scan_i8_kernel<768,32,16,48>": (200, 262181, "default"),
    "scan_tb_kernel<896,16,4,16>": (200, 65573, "default"),
    "scan_tb_kernel<896,16,4,24>": (200, 98341, "default"),
    "scan_tb_kernel<896,16,4,32>": (200, 131109, "default"),
    "scan_tb_kernel<1024,16,4,16>": (61, 163877, "default"),
    "scan_tb_kernel<1024,16,4,24>": (200, 98341, "default"),
    "scan_tb_kernel<1024,16,4,32>": (200, 131109, "default"),
    "scan_i8_kernel<1024,32,16,16>": (200, 131109, "default"),
    "scan_i8_kernel<1024,32,16,32>": (200, 262181, "default"),
}


def family(name):
    return name.split("_kernel")[0]             # scan_tb, scan_wide, scan_i8, scan_f16, scan_w2


def template_args(name):
    return [int(x) for x in name.split("/")[0].split("<")[1].rstrip(">").split(",")]


def is_classic(name):
    return family(name) == "scan_f16" or name.endswith(",-1>")


def is_dump(name):
    return family(name) == "scan_w2" or (family(name) in ("scan_tb", "scan_i8") and template_args(name)[-1] == 0)


def twin_k(name):
    """the smallest k that selects a dump or threshold form (None: the form runs at one k)"""
    if is_classic(name):
        return 1 if template_args(name)[2] == 16 else 17
    return 1 if is_dump(name) else None


def tile_rows_of(name):
    """rows per tile of a form (scan_forms.h: tb_tile_rows, i8_tile_rows, scan_wide_tile_rows, kW1TileRows)"""
    a = template_args(name)
    if family(name) == "scan_wide":
        return 64 if a[1] == 8 and a[0] <= 384 else 32
    return 32 if family(name) == "scan_w2" else a[1]


def chain_slots(name):
    """slots of a scan_tb / scan_i8 register chain (0: the form keeps none)"""
    return max(template_args(name)[-1], 0) if family(name) in ("scan_tb", "scan_i8") else 0


def chain_stride(name):
    """a chain list of the form takes every d-th tile of its workgroup (module docstring)"""
    return 2 if family(name) == "scan_wide" else 1


def parse_plan(text):
    """(streams, query blocks, kp) of a describe text"""
    f = dict(w.split("=") for w in text.split(" + merge")[0].split() if "=" in w)
    return int(f["streams"]), int(f["qblocks"]), int(f["kp"])


def takes_ticket(name, n_rows, streams, qblocks):
    """plan.cpp's finish_plan under TICKET_ENV, restated: chain forms (not int8 rows of 1024 elements), wide forms of 24 / 32
    slots; one query block; four whole rounds at least"""
    a = template_args(name)
    chain = chain_slots(name) > 0 and not (family(name) == "scan_i8" and a[0] > 768)
    wide = family(name) == "scan_wide" and a[2] > 16
    n_tiles = -(-n_rows // tile_rows_of(name))
    return (chain or wide) and qblocks == 1 and n_tiles // streams >= 4


def leg_names(leg):
    return [n for n, c in CASES.items() if c[5] == leg]


# ---- stage 2 of a search: merge.hip's choice among its three regimes, restated
def merge_slice_cand(nq, nlists, k_in):
    m = nlists * k_in
    return 16384 if m <= 16384 and nq * ((m + 8191) // 8192) < 256 else 8192


def merge_regime(nq, nlists, k_in):
    cand = merge_slice_cand(nq, nlists, k_in)
    slices = 1 if nlists * k_in <= cand or k_in > cand else -(-nlists // (cand // k_in))
    return "two-level" if slices > 1 else "64 per thread" if nlists * k_in > 8192 and cand == 16384 else "32 per thread"


# ---- the corpus
PLANTED_AT = (0, 15, 16, 31, 32, 63, 64)
KINDS = ("packed", "chain", "duplicates")


def planted_queries(nq):
    return sorted({q for q in PLANTED_AT + (nq - 1,) if 0 <= q < nq})


def winner_scale(j):
    return 0.95 - 0.004 * (63 - j)


def plant_positions(n, tile_rows, streams, nq, stride=1):
    """{query: (kind, rows)} -- rows in planting order (packed / chain: ascending scale; duplicates: ascending row).  The chains
    take streams 8, 17, 26; the packed runs lie in tiles of streams 29 .. 50, the duplicates in streams 52 .. 63.  Raises
    if two structures want one row all the same."""
    T, S = tile_rows, streams
    n_tiles, n_full = -(-n // T), n // T
    assert n % T >= 3 and S >= 64 and n_tiles > 2 * S, (n, T, S)
    out, taken = {}, set()
    for i, q in enumerate(planted_queries(nq)):
        kind, e = KINDS[i % 3], i // 3
        if kind == "packed":
            a = n_tiles // 2 // S * S + 30 + 8 * e
            rows = list(range(T * a - 3, T * a + 61))
        elif kind == "chain":
            s = (5 + 3 * i) % S
            tiles = [s + stride * j * S for j in range(64) if s + stride * j * S < n_full]
            rows = [t * T + (5 * j + i) % T for j, t in enumerate(tiles)]
        else:
            x = n_tiles // 4 // S * S + 52 + 4 * e
            assert (x + 3) % S != x % S
            rows = sorted([e, x * T + 5, x * T + 6, (x + 1) * T, (x + 3) * T + 7, n - 1 - e])
            assert rows[-1] // T == n_tiles - 1 and rows[-1] >= n_full * T      # inside the ragged last tile
        assert rows and all(0 <= r < n for r in rows) and not (taken & set(rows)), (q, kind)
        taken |= set(rows)
        out[q] = (kind, rows)
    return out


def _unit(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


@functools.lru_cache(maxsize=1)
def _base_rows(pdim, st):
    """the random unit rows of every corpus of this row length and slab type: the longest shard's, shorter ones take a prefix"""
    longest = max([c[3] for c in CASES.values() if (c[1], c[4]) == (pdim, st)] +
                  [v[1] for n, v in LONG_STREAM.items() if CASES[n][1:5:3] == (pdim, st)])
    return _unit(longest, pdim, 1000 + pdim + st)


Corpus = collections.namedtuple("Corpus", "slab scales q16 full64 planted")


def _round_rows(x32, st):
    from oracle import scan_ref
    if st == I8:
        return scan_ref.quantize_rows_i8(x32)
    return x32.astype(np.float16), None


@functools.lru_cache(maxsize=2)
def build_corpus(pdim, st, n, tile_rows, streams, nq, stride):
    """Corpus(slab as it goes to the device, per-row scales or None, fp16 queries, fp64 scores [nq, n] of exactly those numbers
    (read-only), plant_positions' answer)"""
    from oracle import scan_ref
    q16 = (_unit(320, pdim, 2000 + pdim)[:nq] * np.float32(0.995)).astype(np.float16)
    slab, scales = _round_rows(_base_rows(pdim, st)[:n], st)
    planted = plant_positions(n, tile_rows, streams, nq, stride)
    for q, (kind, rows) in planted.items():
        v = q16[q].astype(np.float32)
        if kind == "duplicates":
            x = np.repeat(v[None, :], len(rows), axis=0)
        else:
            x = np.stack([v * np.float32(winner_scale(64 - len(rows) + j)) for j in range(len(rows))])
        r, s = _round_rows(x, st)
        slab[rows] = r
        if s is not None:
            scales[rows] = s
    q64 = scan_ref.dequantized_queries(q16) if st == I8 else q16.astype(np.float64)
    full = np.empty((nq, n), dtype=np.float64)
    for lo in range(0, n, 32768):
        full[:, lo:lo + 32768] = q64 @ slab[lo:lo + 32768].astype(np.float64).T
    if scales is not None:
        full *= scales.astype(np.float64)[None, :]
    full.setflags(write=False)
    c = Corpus(slab, scales, q16, full, planted)
    from topk_check import BAND
    check_reference(c, BAND)      # the precondition of the exact lists, on every corpus that reaches the device
    return c


def corpus_of(name, nq, n, streams):
    """the corpus of one shape of a form; streams is what the planner answers for the shape"""
    return build_corpus(CASES[name][1], CASES[name][4], n, tile_rows_of(name), streams, nq, chain_stride(name))


def check_reference(c, band):
    """What lets the device test demand exact lists on the planted queries, on the reference alone: every |score| <= 1, the
    planted rows of a query 10 bands clear of each other and of every other row, duplicates bit-equal."""
    assert np.abs(c.full64).max() <= 1.0
    for q, (kind, rows) in c.planted.items():
        s = c.full64[q]
        rest = np.delete(s, rows).max()
        if kind == "duplicates":
            assert (s[rows] == s[rows[0]]).all(), (q, s[rows])
            assert s[rows[0]] - rest >= 10 * band, (q, kind, s[rows[0]], rest)
        else:
            assert (np.diff(s[rows]) >= 10 * band).all(), (q, kind, np.diff(s[rows]).min())
            assert s[rows[0]] - rest >= 10 * band, (q, kind, s[rows[0]], rest)


def expected_prefix(c, q, k):
    """the head of query q's list that is exact: the planted rows that lead the fp64 order (ties by id), at most k"""
    kind, rows = c.planted[q]
    order = np.lexsort((np.asarray(rows), -c.full64[q, rows]))
    return np.asarray(rows)[order][:k]


# ---- one search on the device
class _Env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {n: os.environ.get(n) for n in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for n, v in self.old.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v


_ON_DEVICE = collections.OrderedDict()    # id(Corpus) -> (Corpus, slab, scales, queries): the last corpus stays on the device


def _device(c, cuda):
    import torch
    hit = _ON_DEVICE.get(id(c))
    if hit is None:
        _ON_DEVICE.clear()
        hit = (c, torch.from_numpy(c.slab).to(cuda), torch.from_numpy(c.scales).to(cuda) if c.scales is not None else None,
               torch.from_numpy(c.q16).to(cuda))
        _ON_DEVICE[id(c)] = hit
    return hit[1:]


def plan_of(name, nq, n, k, env):
    """(streams, query blocks, kp) the library plans for the shape; the describe text must name the form"""
    from rag import _native as nat
    with _Env(env):
        text = nat.scan_plan_describe(nq, CASES[name][1], k, n, slab_type=CASES[name][4])
    assert text.startswith(name.split("/")[0]), (name, (nq, n, k), env, text)
    return parse_plan(text)


def search(name, c, cuda, k, env, id_base=0):
    """-> (scores, ids, first word of the poisoned workspace after the launch); asserts the describe text first"""
    import torch
    from rag import _native as nat
    nq, n = c.full64.shape
    dim, st = CASES[name][1], CASES[name][4]
    plan_of(name, nq, n, k, env)
    slab, scales, q = _device(c, cuda)
    with _Env(env):
        ws = torch.full((nat.scan_workspace_bytes(nq, dim, k, n),), POISON, dtype=torch.uint8, device=cuda)
        sc, ids = nat.cosine_topk(q, slab, n, dim, k, slab_type=st, scales=scales, id_base=id_base, workspace=ws)
        torch.cuda.synchronize()
    return sc.cpu().numpy(), ids.cpu().numpy(), int(ws[:4].view(torch.int32)[0])


POISON_WORD = int(np.array([POISON] * 4, dtype=np.uint8).view(np.int32)[0])
RATIOS = {}         # family -> worst |score - fp64| / TIGHT_TOL seen by this process (and, in the parent, by its children)
CASE_RATIOS = []    # (ratio, "form k= nq= n=") of every checked launch


def check_lists(name, c, sc, ids, k):
    """check_topk over all queries, then the planted queries exactly; records the score ratio"""
    from topk_check import TIGHT_TOL, check_topk
    nq, n = c.full64.shape
    ratio = float(np.abs(np.take_along_axis(c.full64, np.clip(ids, 0, n - 1), 1) - sc).max() / TIGHT_TOL)
    RATIOS[family(name)] = max(RATIOS.get(family(name), 0.0), ratio)
    CASE_RATIOS.append((ratio, "%s k=%d nq=%d n=%d" % (name, k, nq, n)))
    check_topk(sc, ids, c.full64, k)
    for q, (kind, rows) in c.planted.items():
        want = expected_prefix(c, q, k)
        assert np.array_equal(ids[q][:len(want)], want), (name, k, q, kind, ids[q].tolist(), want.tolist())
        if kind == "duplicates":
            assert (sc[q][:len(want)] == sc[q][0]).all(), (name, k, q, sc[q].tolist())


def run_shape(name, nq, n, cuda, env, first=False):
    """One shape of a form at the form's largest k.  first: the form's own case, which also runs its smallest k where it has
    one, the ticketed schedule where the plan allows it and id_base where the form speaks for its family."""
    k = CASES[name][2]
    streams, qblocks, _ = plan_of(name, nq, n, k, env)
    if chain_slots(name) and (name in LONG_STREAM) != first:      # the shape that is there to fill the chain and overflow it
        assert -(-n // tile_rows_of(name)) // streams > chain_slots(name), (name, nq, n, streams)
    c = corpus_of(name, nq, n, streams)
    sc, ids, word = search(name, c, cuda, k, env)
    check_lists(name, c, sc, ids, k)
    if not first:
        return
    if takes_ticket(name, n, streams, qblocks):
        assert word == POISON_WORD, (name, "a static launch leaves the workspace's first word alone", word)
        ts, ti, tword = search(name, c, cuda, k, dict(env, **TICKET_ENV))
        assert 0 < tword < n, (name, "no ticket was drawn", tword)
        assert np.array_equal(ti, ids) and np.array_equal(ts.view(np.int32), sc.view(np.int32)), (name, "ticketed != static")
    if twin_k(name) is not None:
        s1, i1, _ = search(name, c, cuda, twin_k(name), env)
        check_lists(name, c, s1, i1, twin_k(name))
    if name in ID_BASE_FORMS:
        bs, bi, _ = search(name, c, cuda, k, env, id_base=ID_BASE)
        assert np.array_equal(bi, np.where(ids >= 0, ids + ID_BASE, -1)) and np.array_equal(bs.view(np.int32), sc.view(np.int32)), name


def process_of(leg):
    """the process a leg's shapes run in: a child per leg of CHILD_LEGS, the test process ("default") for the others"""
    return leg if leg in CHILD_LEGS else "default"


def run_form(name, cuda, env):
    """Everything one form is asked in the process of its own leg: its case, then its second shapes -- above the bootstrap, two
    query blocks, the long stream where that needs no other process."""
    nq, dim, k, n, st, leg = CASES[name]
    run_shape(name, nq, n, cuda, env, first=True)
    for second in (BOOT_ABOVE, MULTI_BLOCK):
        if name in second:
            run_shape(name, second[name][0], second[name][1], cuda, env)
    if name in LONG_STREAM and process_of(LONG_STREAM[name][2]) == process_of(leg):
        run_shape(name, LONG_STREAM[name][0], LONG_STREAM[name][1], cuda, env)


def long_streams_from_elsewhere(process):
    """the forms whose long-stream shape needs this process's knobs while their own case runs in another process"""
    return [n for n, (_, _, leg) in LONG_STREAM.items() if process_of(leg) == process != process_of(CASES[n][5])]


ID_BASE_FORMS = {next(n for n in CASES if family(n) == f) for f in ("scan_tb", "scan_wide", "scan_i8", "scan_f16", "scan_w2")}


def main(argv):
    """A leg's forms in a fresh process (the knobs of CHILD_LEGS and CRS_SCAN_VARIANT are read once per process):
         python tests/_scan_form_cases.py <leg> [f16-classic]
    under the leg's environment, set by the caller.  One line per form, "PASS <name>" ("PASS long <name>" for the long-stream
    shapes of other legs' forms), then the ratios.  The first failed check or HIP error ends the run: nothing more goes to a
    device that has returned a wrong list."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "compressed-rag-suite_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    assert torch.cuda.is_available(), "no ROCm device is visible"
    cuda = torch.device("cuda:0")
    jobs = [("", n) for n in leg_names(argv[1])]
    if len(argv) > 2 and argv[2] == "f16-classic":
        jobs = [j for j in jobs if family(j[1]) == "scan_f16"]
    else:
        jobs += [("long ", n) for n in long_streams_from_elsewhere(argv[1])]
    status = 0
    for what, name in jobs:
        try:
            if what:
                run_shape(name, LONG_STREAM[name][0], LONG_STREAM[name][1], cuda, {})
            else:
                run_form(name, cuda, {})
            print("PASS " + what + name, flush=True)
        except AssertionError as e:
            print("FAIL %s%s: %s" % (what, name, str(e)[:600].replace("\n", " ")), flush=True)
            status = 1
            break
        except Exception as e:      # a HIP error
            print("ABORT %s%s: %r" % (what, name, e), flush=True)
            status = 3
            break
    for fam, r in sorted(RATIOS.items()):
        print("RATIO %s %.4f" % (fam, r), flush=True)
    for r, what in CASE_RATIOS:
        print("CASE %.4f %s" % (r, what), flush=True)
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv))
