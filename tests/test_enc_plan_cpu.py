"""No GPU: the encoder's planner (csrc/enc_plan.cpp, csrc/enc_forms.h) as the stand-alone program tools/enc_plan_table.cpp, built here
with g++ -fsanitize=address,undefined (host code in a program of its own).

1. Against tests/golden/enc_plans.json.xz -- a rocprofv3 kernel trace of every call of tools/enc_case_kernels.py::calls and the
   answers of crs_encoder_workspace_bytes, recorded on an MI355X (256 CUs) before the planner existed, one fresh process per knob
   setting -- the planner reproduces every launch list (kernel with template arguments, grid in workgroups, workgroup size) and
   every byte count.  The trace's LDS column holds a kernel's STATIC LDS only (0 for the kernels that size theirs at launch), so the
   plans' dynamic LDS is checked by 3. and 4. instead.
2. The kernel names of every case of _encoder_cases.ALL_CASES (what profiles/enc_cases_kernels.txt lists) are the golden's.
3. Invariants of every plan over hidden 64..1024, head_dim 16 / 32 / 64, ffn = 4 hidden and the cases' other ffn values, the golden's
   token counts and sequence lengths, both flag values.
4. Fields worked out by hand from the code as it stood before; each derivation is in its test's docstring.
5. Coverage: every (step, family / form) pair the default knobs can produce over the grid of 3. is reached by a case of the fp64
   suites, or listed in UNREACHED with the reason."""
import json
import lzma
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _crossenc_cases as cc  # noqa: E402
import _encoder_cases as ec  # noqa: E402
import _mpnet_cases as mc  # noqa: E402
import enc_case_kernels as eck  # noqa: E402

CSRC = os.path.join(ROOT, "compressed-rag-suite_amd", "csrc")
GEMM_FIELDS = "family slabs tm kc kin persist items ksplit colblocks streams".split()
STEPS = ("qkv", "up", "out", "down")
MAX_LDS = 160 * 1024
LN_SLABS = {1, 2, 3, 4, 6, 8, 16}        # csrc/enc_forms.h: CRS_LN_SLABS


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("enc_plan") / "enc_plan_table")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tools", "enc_plan_table.cpp"), os.path.join(CSRC, "enc_plan.cpp")], check=True, timeout=300)

    def run(cases, cus=256, env=None):
        """cases: ("fwd", hidden, heads, ffn, flags, batch, seq, rel_bias, pair) or ("gemm", m, n, k, mode) -> one dict per case"""
        e = {k: v for k, v in os.environ.items() if not k.startswith("CRS_")}
        e["ASAN_OPTIONS"] = "detect_leaks=0"      # the planner allocates nothing; the leak check at exit cannot run under a tracer
        e.update(env or {})
        r = subprocess.run([exe, str(cus)], input="".join(" ".join(map(str, c)) + "\n" for c in cases), env=e, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out = r.stdout.splitlines()
        assert len(out) == len(cases)
        rows = []
        for line in out:
            fields, text = line.split("\t")
            row = {"text": [t for t in text.split(";") if t]}
            for kv in fields.split():
                k, v = kv.split("=")
                row[k] = dict(zip(GEMM_FIELDS, [f if i == 0 else int(f) for i, f in enumerate(v.split("/"))])) if "/" in v else \
                    (v if k == "attn" else int(v))
            rows.append(row)
        return rows
    return run


@pytest.fixture(scope="module")
def golden():
    with lzma.open(eck.GOLDEN, "rt") as f:
        return json.load(f)


def call_line(c):
    if c["kind"] == "gemm":
        return ("gemm", c["m"], c["n"], c["k"], c["mode"])
    return ("fwd", c["hidden"], c["heads"], c["ffn"], c["small"], c["batch"], c["seq"], c["rel"], c["pair"])


def no_lds(line):
    return re.sub(r" lds=\d+$", "", line)


def whole_forward(text, layers):
    """the describe text holds embedding, ONE layer and the tail"""
    return text[:1] + text[1:-1] * layers + text[-1:]


SETTINGS = [{}, {"CRS_ATTN_SEQ": "0"}, {"CRS_ATTN_X32": "0"}, {"CRS_ATTN_SHORT": "0"}, {"CRS_ATTN_QT": "4"}, {"CRS_ROWLN2_VARIANT": "0"},
            {"CRS_ENC_BIGLN": "0"}, {"CRS_GEMM8": "0"}, {"CRS_ENC_QKVATTN": "0", "CRS_PANEL_KC": "128"},
            {"CRS_ENC_PANEL_MULTI": "0", "CRS_PANEL_KC": "384"}, {"CRS_PANEL_MAX_SPLIT": "2"}, {"CRS_GEMM_BIG": "0"}, {"CRS_GEMM_STREAM": "0"}]


def test_golden_holds_the_calls_and_the_settings(golden):
    """the default setting has every call (small-LDS, relative-bias and pair forwards included), the others the cases, both grids and
    the GEMM shapes; both sides of every threshold are in the default setting's token grid"""
    assert golden["cus"] == 256
    assert [s["env"] for s in golden["settings"]] == SETTINGS
    strip = lambda cs: [{k: v for k, v in c.items() if k != "list"} for c in cs]
    assert strip(golden["settings"][0]["calls"]) == eck.calls("full")
    for s in golden["settings"][1:]:
        assert strip(s["calls"]) == eck.calls("grid")
    assert golden["bytes_tokens"] == eck.BYTES_TOKENS and set(golden["settings"][0]["bytes"]) == {n for n, _ in eck.grid_models()}
    assert {1024, 1040, 2048, 2064, 4096, 4112} <= set(eck.GRID_TOKENS)


@pytest.mark.parametrize("setting", range(len(SETTINGS)))
def test_planner_reproduces_the_golden_launches_and_byte_counts(table, golden, setting):
    s = golden["settings"][setting]
    rows = table([call_line(c) for c in s["calls"]], cus=golden["cus"], env=s["env"])
    bad = []
    for c, r in zip(s["calls"], rows):
        want = [no_lds(golden["texts"][i]) for i in golden["lists"][c["list"]]]
        got = [no_lds(t) for t in (whole_forward(r["text"], c["layers"]) if c["kind"] == "fwd" else r["text"])]
        if got != want:
            bad.append((c["name"], c.get("small"), got, want))
    assert not bad, "%d of %d calls differ under %s, first: %s" % (len(bad), len(rows), s["env"], bad[:2])
    models = dict(eck.grid_models())
    for name, idx in s["bytes"].items():
        cfg = models[name]
        rows = table([("fwd", cfg.hidden, cfg.heads, cfg.ffn, 0, t // 16, 16, 0, 0) for t in golden["bytes_tokens"]], cus=golden["cus"], env=s["env"])
        assert [r["total"] for r in rows] == [golden["sizes"][i] for i in idx], (name, s["env"])


def test_kernel_names_of_every_case(table, golden):
    """what profiles/enc_cases_kernels.txt lists: each kernel once, in first-launch order"""
    calls = {c["name"]: c for c in golden["settings"][0]["calls"] if not c.get("small")}
    rows = table([("fwd", c.cfg.hidden, c.cfg.heads, c.cfg.ffn, 0, c.batch, c.seq, 0, 0) for c in ec.ALL_CASES])
    uniq = lambda names: list(dict.fromkeys(names))
    for case, r in zip(ec.ALL_CASES, rows):
        want = uniq(golden["texts"][i].split(" grid=")[0] for i in golden["lists"][calls["case:" + case.name]["list"]])
        assert uniq(t.split(" grid=")[0] for t in r["text"]) == want, case.name


# ---------------------------------------------------------------------------------------------------------------------
OTHER_FFN = {384: (1088, 2304), 512: (3072, 1152), 768: (6144,)}      # the cases' ffn values that are not 4 x hidden


def grid_cases(flags=(0, 1)):
    shapes = [(t // 16, 16) for t in eck.GRID_TOKENS] + [(4, s) for s in eck.GRID_SEQS]
    return [("fwd", h, h // hd, f, fl, b, s, 0, 0) for h in range(64, 1025, 64) for hd in (16, 32, 64) for f in (4 * h,) + OTHER_FFN.get(h, ())
            for fl in flags for b, s in shapes]


def step_k(case, step):
    return case[3] if step == "down" else case[1]


@pytest.mark.parametrize("cus", [256, 64])
def test_every_plan_keeps_the_invariants(table, cus):
    cases = grid_cases()
    seen = set()
    for c, r in zip(cases, table(cases, cus=cus)):
        tokens = c[5] * c[6]
        assert r["attn_lds"] <= MAX_LDS and (r["attn"] == "Fused") == (r["qkv"]["family"] == "None"), (c, r)
        for step in STEPS:
            g, k = r[step], step_k(c, step)
            fam = g["family"]
            seen.add(fam)
            if step in ("out", "down") and r[step + "_rowln2"]:
                assert fam == "None" and c[1] == 384 and tokens > 4096
                continue
            if fam == "None":
                assert step == "qkv"
                continue
            assert r[step + "_wgs"] >= 1 and 0 <= r[step + "_lds"] <= MAX_LDS, (c, step, r)
            assert g["slabs"] in LN_SLABS and (g["slabs"] == 1 or step in ("out", "down")), (c, step, g)
            assert r["max_split"] >= g["slabs"], (c, step, r)                 # the workspace's y32 holds every slab written
            if fam == "Panel":
                assert g["tm"] in (64, 128) and g["kc"] in (128, 256, 384) and k % g["kc"] == 0 and g["kin"] * g["slabs"] * g["kc"] == k, (c, step, g)
                assert r[step + "_lds"] <= (48 * 1024 if c[4] else MAX_LDS)     # CRS_ENC_SMALL_LDS: 128-column chunks
            if fam in ("Gemm8", "Gemm8SplitK"):
                assert tokens % 256 == 0 and g["items"] >= 1 and g["ksplit"] * g["slabs"] == k, (c, step, g)
                assert r[step + "_wgs"] == (cus if g["persist"] else g["items"])
            if fam == "Gemm8SplitK":
                assert g["slabs"] > 1 and g["ksplit"] >= 256 and g["ksplit"] % 128 == 0, (c, step, g)
            if fam in ("Stream", "StreamKS"):
                assert step in ("qkv", "up") and 1 <= g["streams"] and r[step + "_wgs"] == g["colblocks"] * g["streams"], (c, step, g)
                assert (fam == "StreamKS") == (k == 768)
    assert {"Tiled", "Panel", "Stream", "Big", "Gemm8", "Gemm8SplitK"} <= seen


def test_gemm_entry_invariants(table):
    """crs_gemm_f16: stream-KS only in modes 0 / 1, nothing but modes 0..2, gemm8 on whole 256-row tiles"""
    cases = [("gemm", m, n, k, mode) for m in (1, 64, 511, 512, 4096, 32768) for n in (64, 384, 512, 768, 2304) for k in (64, 128, 384, 768, 3072)
             for mode in (0, 1, 2)]
    for c, r in zip(cases, table(cases)):
        g = r["gemm"]
        assert g["family"] != "None" and g["family"] != "Panel" and r["gemm_wgs"] >= 1 and r["gemm_lds"] <= MAX_LDS, (c, r)
        assert g["family"] != "StreamKS" or (c[4] in (0, 1) and c[3] == 768)
        assert g["family"] != "Gemm8" or c[1] % 256 == 0
    assert table([("gemm", 512, 512, 768, 3)])[0]["gemm"]["family"] == "None"


# ---------------------------------------------------------------------------------------------------------------------
BGE = (768, 12, 3072)
MINI = (384, 12, 1536)


def test_bge_base_at_2048_tokens_sizes_six_slabs_and_writes_two(table):
    """bge-base, 128 x 16 = 2048 tokens.  The workspace rule takes the largest of: the panel slabs of FFN-down (K = 3072 = 8 chunks of
    384, halved to the cap of 2 above 1024 tokens: 2) and of the out-projection (768 = 2 chunks: 2), and gemm8_splitk of both shapes
    whether or not the panel path takes them first -- 2048 rows are 8 x 3 = 24 tiles of 256 x 256, < 128, and the first slab count with
    24 s >= 128 whose slabs are >= 256 columns in multiples of 128 is 6 (3072 / 6 = 512) for FFN-down, none for K = 768.  So y32 is sized
    for 6 slabs while the forward, on the panel path at <= 2048 tokens, writes 2: an upper bound.  Bytes: x32 6 291 456, y32 six times
    that, x16 and ctx 3 145 728 each, qkv 9 437 184, ffn 12 582 912, all multiples of 256."""
    r, = table([("fwd",) + BGE + (0, 128, 16, 0, 0)])
    assert r["max_split"] == 6 and r["out"]["slabs"] == 2 and r["down"]["slabs"] == 2
    assert r["out"]["family"] == r["down"]["family"] == "Panel"
    assert r["total"] == 6_291_456 * 7 + 3_145_728 * 2 + 9_437_184 + 12_582_912
    # one token block further the multi-chunk contractions leave the panel kernel: tiled mode 2, one slab; 2064 is no multiple of 256
    r, = table([("fwd",) + BGE + (0, 129, 16, 0, 0)])
    assert (r["max_split"], r["out"]["family"], r["down"]["family"], r["down"]["slabs"]) == (1, "Tiled", "Tiled", 1)


def test_minilm_query_batch(table):
    """MiniLM (384 / 12 heads / 1536), 8 x 16 = 128 tokens.  Fused QKV + attention: head_dim 32, LDS = (64 + 96) x 384 x 2 for the x16 and
    weight panels + (2 x 64 x 40 + 32 x 72) x 2 for Q, K, V^T + 4 x 16 x 72 x 2 for P = 122 880 + 14 848 + 9216 = 146 944; grid 2 token
    blocks x 12 heads.  Out-projection: K = 384 is one chunk, one slab; 6 column blocks x 2 row tiles of 64 = 12 workgroups <= 256: 64-row
    tiles, the chunk stays 384, LDS (64 + 64) x 384 x 2 = 98 304.  FFN-up: 24 x 2 workgroups, the same LDS.  FFN-down: 1536 = 4 chunks = 4 slabs
    (cap 4 up to 1024 tokens), 6 x 2 x 4 = 48 workgroups, kin 1.  With CRS_ENC_SMALL_LDS: no fused kernel; QKV on the panel kernel in
    128-column chunks (kin 3, LDS 128 x 128 x 2 = 32 768) and the query-length attention kernel."""
    r, = table([("fwd",) + MINI + (0, 8, 16, 0, 0)])
    assert (r["attn"], r["attn_lds"], r["qkv"]["family"]) == ("Fused", 146_944, "None")
    assert r["text"][1] == "qkv_attn_kernel<32> grid=2x12x1 wg=512x1x1 lds=146944"
    assert (r["out"]["family"], r["out"]["slabs"], r["out"]["tm"], r["out"]["kc"], r["out"]["kin"], r["out_lds"], r["out_wgs"]) == ("Panel", 1, 64, 384, 1, 98_304, 12)
    assert (r["up"]["family"], r["up"]["kc"], r["up_lds"], r["up_wgs"]) == ("Panel", 384, 98_304, 48)
    assert (r["down"]["slabs"], r["down"]["kc"], r["down"]["kin"], r["down_wgs"], r["max_split"]) == (4, 384, 1, 48, 4)
    assert r["text"][-2:] == ["layernorm2_kernel<3, 4> grid=32x1x1 wg=256x1x1 lds=0", "pool_kernel grid=8x1x1 wg=256x1x1 lds=0"]
    r, = table([("fwd",) + MINI + (1, 8, 16, 0, 0)])
    assert (r["attn"], r["qkv"]["family"], r["qkv"]["kc"], r["qkv"]["kin"], r["qkv_lds"]) == ("Short", "Panel", 128, 3, 32_768)
    assert r["text"][2] == "attention_short_kernel<32> grid=24x1x1 wg=256x1x1 lds=0"


def test_bge_base_panel_tiles_and_chunks(table):
    """bge-base, 64 x 16 = 1024 tokens.  QKV: N = 2304 = 36 column blocks; 64-row tiles would be 36 x 16 = 576 workgroups > 256, so
    128-row tiles: 36 x 8 = 288 > 256 still, so the 384-column chunk is staged in 128-column pieces: kc 128, kin 768 / 128 = 6, LDS
    (128 + 64) x 128 x 2 = 49 152.  FFN-down: 8 chunks, cap 4 at <= 1024 tokens: 4 slabs, 12 x 8 x 4 = 384 workgroups > 256: kc 128,
    kin = (3072 / 384 / 4) x 3 = 6, and 6 x 4 x 128 = 3072.  CRS_PANEL_KC=384 keeps the one-shot chunk: kin 2, LDS 147 456."""
    case = ("fwd",) + BGE + (0, 64, 16, 0, 0)
    r, = table([case])
    assert (r["qkv"]["family"], r["qkv"]["tm"], r["qkv"]["kc"], r["qkv"]["kin"], r["qkv_lds"], r["qkv_wgs"]) == ("Panel", 128, 128, 6, 49_152, 288)
    assert (r["down"]["slabs"], r["down"]["tm"], r["down"]["kc"], r["down"]["kin"], r["down_wgs"]) == (4, 128, 128, 6, 384)
    assert r["attn"] == "Short"
    r, = table([case], env={"CRS_PANEL_KC": "384"})
    assert (r["down"]["kc"], r["down"]["kin"], r["down_lds"]) == (384, 2, 147_456)


def test_bge_base_index_build_side(table):
    """bge-base at 4096 tokens (16 x 256) on 256 CUs.  QKV 4096 x 2304 x 768: 16 x 9 = 144 tiles of 256 x 256 >= 128: the phase-scheduled
    kernel, 144 items <= 256 CUs: one workgroup per item, LDS 2 x 64 KB + 8 x 2304 = 149 504.  FFN-up: 16 x 12 = 192 items.  Both
    projections back to 768 columns: 4096 tokens are over the split-K panel limit (multi-chunk K), 16 x 3 = 48 tiles < 128: split-K with the
    first of 2, 3, 4, 6, 8 that reaches 128 workgroups: 3 (144), slabs of 256 / 1024 columns.  Attention: head_dim 64, seq 256: the 16x16x32
    whole-sequence kernel <64, 256, 4, 2>, LDS (256 x 72 + 64 x 264) x 2 = 70 656.  On 64 CUs the fp16-epilogue launches are persistent:
    64 workgroups.  32 768 tokens: 1152 / 1536 items, persistent on 256 CUs; the fp32 + residual projections (128 x 3 = 384 tiles) take the
    whole-K phase-scheduled kernel, one workgroup per item."""
    case = ("fwd",) + BGE + (0, 16, 256, 0, 0)
    r, = table([case])
    assert (r["qkv"]["family"], r["qkv"]["persist"], r["qkv"]["items"], r["qkv_wgs"], r["qkv_lds"]) == ("Gemm8", 0, 144, 144, 149_504)
    assert (r["up"]["family"], r["up"]["items"]) == ("Gemm8", 192)
    assert (r["out"]["family"], r["out"]["slabs"], r["out"]["ksplit"], r["out"]["items"]) == ("Gemm8SplitK", 3, 256, 144)
    assert (r["down"]["family"], r["down"]["slabs"], r["down"]["ksplit"], r["max_split"]) == ("Gemm8SplitK", 3, 1024, 3)
    assert (r["attn"], r["attn_lds"]) == ("Seq32", 70_656) and r["text"][2].startswith("attention_seq32_kernel<64, 256, 4, 2> grid=192x1x1 wg=256x1x1")
    r, = table([case], cus=64)
    assert (r["qkv"]["persist"], r["qkv_wgs"], r["out"]["persist"], r["out_wgs"]) == (1, 64, 0, 144)
    r, = table([("fwd",) + BGE + (0, 2048, 16, 0, 0)])
    assert (r["qkv"]["persist"], r["qkv"]["items"], r["qkv_wgs"], r["up"]["items"]) == (1, 1152, 256, 1536)
    assert (r["out"]["family"], r["out"]["persist"], r["out"]["items"], r["out"]["slabs"]) == ("Gemm8", 0, 384, 1)


def test_minilm_index_build_side(table):
    """MiniLM at 4640 tokens (29 x 160): over 4096 tokens and hidden 384: both projections + LayerNorm are the pipelined kernel, 37 blocks of
    128 rows, 128 KB of LDS, the two-stage variant unless CRS_ROWLN2_VARIANT=0.  QKV 4640 x 1152 x 384: 4640 is no multiple of 256 and K < 512:
    the row-streaming kernel; 9 column blocks of 128, 2 x 256 / 9 = 56 streams (a multiple of 8), 504 workgroups, LDS 2 x 32 x 384 x 2 + 4 x 32
    x 40 x 2 = 59 392.  FFN-up: 12 column blocks, 42 -> 40 streams.  CRS_GEMM_STREAM=0: the tiled kernel, 9 x 37 tiles."""
    case = ("fwd",) + MINI + (0, 29, 160, 0, 0)
    r, = table([case])
    assert (r["out_rowln2"], r["down_rowln2"], r["rowln2_variant"]) == (1, 1, 1)
    assert r["text"][3] == "gemm_rowln2_kernel<64, 2> grid=37x1x1 wg=512x1x1 lds=131072"
    assert (r["qkv"]["family"], r["qkv"]["colblocks"], r["qkv"]["streams"], r["qkv_wgs"], r["qkv_lds"]) == ("Stream", 9, 56, 504, 59_392)
    assert (r["up"]["colblocks"], r["up"]["streams"]) == (12, 40)
    r, = table([case], env={"CRS_GEMM_STREAM": "0", "CRS_ROWLN2_VARIANT": "0"})
    assert (r["qkv"]["family"], r["qkv_wgs"], r["rowln2_variant"]) == ("Tiled", 333, 0)


def test_stream_ks_is_reached_through_the_gemm_entry_only(table):
    """K = 768 streams in the K-split form (fp16 outputs): crs_gemm_f16 at 512 x 512 x 768 takes it -- 4 column blocks, one workgroup per CU:
    256 / 4 = 64 streams, cut to the 16 row tiles: 64 workgroups of 512, LDS 2 x 32 x 768 x 2 + 10 240 + 32 768 = 141 312.  No default forward does: with hidden 768
    every fp16-epilogue projection up to 4096 tokens is a multi-chunk panel, and from 4112 tokens (>= 17 row blocks x 9 column blocks of 256)
    the 256-row kernels have their 128 workgroups.  CRS_ENC_PANEL_MULTI=0 sends the query-batch sizes there."""
    r, = table([("gemm", 512, 512, 768, 0)])
    assert (r["gemm"]["family"], r["gemm"]["colblocks"], r["gemm"]["streams"], r["gemm_wgs"], r["gemm_lds"]) == ("StreamKS", 4, 16, 64, 141_312)
    assert r["text"] == ["gemm_stream_ks_kernel<768, 0> grid=64x1x1 wg=512x1x1 lds=141312"]
    cases = [c for c in grid_cases() if c[1] == 768]
    assert not any(r[s]["family"] == "StreamKS" for r in table(cases) for s in STEPS)
    r, = table([("fwd",) + BGE + (0, 64, 16, 0, 0)], env={"CRS_ENC_PANEL_MULTI": "0"})
    assert r["qkv"]["family"] == "StreamKS" and r["up"]["family"] == "StreamKS"


# ---------------------------------------------------------------------------------------------------------------------
def pairs_of(case, r):
    out = {("attn", r["attn"])}
    for step in STEPS:
        fam = "Rowln2" if step in ("out", "down") and r[step + "_rowln2"] else r[step]["family"]
        if fam == "Panel":
            fam += "/%d" % r[step]["tm"]
        if fam == "Gemm8":
            fam += "/persistent" if r[step]["persist"] else ""
        out.add((step, fam))
    return out


# (step, family / form) pairs of the grid that no forward of the fp64 suites reaches, with the reason
UNREACHED = {}


def test_every_reachable_form_is_reached_by_a_case(table):
    grid = grid_cases()
    possible = {}
    for c, r in zip(grid, table(grid)):
        for p in pairs_of(c, r):
            if p not in possible or c[5] * c[6] < possible[p][5] * possible[p][6]:
                possible[p] = c
    suite = []
    for c in ec.ALL_CASES:
        suite += [("fwd", c.cfg.hidden, c.cfg.heads, c.cfg.ffn, fl, c.batch, c.seq, 0, 0) for fl in ((0, 1) if c.query_batch else (0,))]
    suite += [("fwd", cfg.hidden, cfg.heads, cfg.ffn, fl, b, s, 1, 0) for _, cfg, _, b, s in mc.CASES for fl in (0, 1)]
    suite += [("fwd", cfg.hidden, cfg.heads, cfg.ffn, 0, b, s, 0, 1) for _, cfg, _, b, s in cc.CASES]
    reached = set()
    for c, r in zip(suite, table(suite)):
        reached |= pairs_of(c, r)
    missing = {p: c for p, c in possible.items() if p not in reached and p not in UNREACHED}
    assert not missing, "forms no case reaches (pair: smallest grid case): %s" % missing
    assert not set(UNREACHED) & reached, "listed as unreached but reached: %s" % (set(UNREACHED) & reached)
