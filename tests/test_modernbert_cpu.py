"""No GPU: what loading ModernBERT encoders adds on the host -- the fp64 numpy restatement of the forward against
transformers.ModernBertModel (tests/golden/encoder_modernbert.npz, tools/make_modernbert_golden.py), the window rule, the Wi
interleave, the two name dialects and every refused option, the planner's new lines, the new symbols, the byte-level BPE tokeniser
fixture, and for each new kernel an fp32 emulation inside its derived bound with planted faults far outside it."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _attn_ref as ar
import _attn_win_ref as aw
import _gated_gelu_ref as gg
import _gated_ref as gt
import _gemm_ref as gr
import _modernbert_cases as mc
import _row_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "compressed-rag-suite_amd", "csrc")
WIDE = 30.0          # "by a wide margin": a planted fault must leave its bound by at least this factor


@pytest.fixture(scope="module")
def golden():
    return np.load(mc.GOLDEN)


# ---- the model -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [c[0] for c in mc.CASES])
def test_restatement_reproduces_transformers_in_fp64(golden, key):
    """encode_ref with the angles transformers itself uses (fp32, whatever the model's dtype) against ModernBertModel in fp64: 1e-9.
    With the exact fp64 angles -- what the library's host code builds -- the hidden states move by the fp32 angles' error only."""
    _, cfg, seed, lens, seq = next(c for c in mc.CASES if c[0] == key)
    z = golden
    assert int(z[key + ".seed"]) == seed and z[key + ".ids"].shape == (len(lens), seq)
    ids, mask = z[key + ".ids"], z[key + ".mask"].astype(np.int32)
    assert mask.sum(1).tolist() == list(lens)
    w = mc.make_weights(cfg, seed)
    real = mask.astype(bool)
    same = mc.encode_ref(ids, mask, w, cfg, fp32_angles=True)
    exact = mc.encode_ref(ids, mask, w, cfg)
    assert np.isfinite(same).all()                               # padding rows too: a query without any allowed key is a zero row
    print(key, float(np.abs(same[real] - z[key + ".hidden"]).max()), float(np.abs(exact[real] - z[key + ".hidden"]).max()))
    assert np.abs(same[real] - z[key + ".hidden"]).max() < 1e-9
    assert np.abs(exact[real] - z[key + ".hidden"]).max() < 1e-4
    mean, cls = mc.pooled(same, mask)
    assert np.abs(mean - z[key + ".mean_norm"]).max() < 1e-9 and np.abs(cls - z[key + ".cls_norm"]).max() < 1e-9


def test_window_rule_is_inclusive_at_both_ends_and_it_bites(golden):
    m = mc.window_mask(40, 8)
    assert m[20, 12] and m[20, 28] and not m[20, 11] and not m[20, 29] and m[0, 8] and not m[0, 9]
    assert (m == m.T).all() and m.sum(1).max() == 17
    # the golden separates the rule from its neighbours: a window one key shorter or longer at one end moves the hidden states
    key, cfg, seed, lens, seq = mc.CASES[1]
    w = mc.make_weights(cfg, seed)
    ids, mask = golden[key + ".ids"], golden[key + ".mask"].astype(np.int32)
    real = mask.astype(bool)
    i = np.arange(seq)
    d = i[None, :] - i[:, None]                                  # key - query
    for name, rule in (("short right", (d <= 7) & (d >= -8)), ("long left", (d <= 8) & (d >= -9)), ("exclusive", np.abs(d) < 8)):
        h = mc.encode_ref(ids, mask, w, cfg, fp32_angles=True, window_rule=lambda s, wd, r=rule: r)
        moved = np.abs(h[real] - golden[key + ".hidden"]).max()
        print(name, float(moved))
        assert moved > 3e-2                                      # the GPU test's hidden-state bound


def test_changing_one_token_moves_exactly_the_rows_of_its_window():
    """One sliding layer (layer 1 of a two-layer model with global_every = 2), fed the SAME residual stream except at token 20: its
    attention output differs in rows 12 .. 28 and nowhere else."""
    import math
    cfg = mc.MbCfg("two", 300, 64, 2, 4, 128, 256, 160, global_every=2)
    w = {k: np.asarray(v, dtype=np.float64) for k, v in mc.make_weights(cfg, 9).items()}
    rng = np.random.default_rng(10)
    r = rng.standard_normal((1, 48, 64))
    r2 = r.copy()
    r2[0, 20] += rng.standard_normal(64)
    hd, nh = 16, 4
    cos, sin = mc.rope_cos_sin(48, hd, mc.LOCAL_THETA)
    cos, sin = np.concatenate([cos, cos], 1)[None, None], np.concatenate([sin, sin], 1)[None, None]

    def attn(x):
        mu, var = x.mean(-1, keepdims=True), x.var(-1, keepdims=True)
        x = (x - mu) / np.sqrt(var + cfg.norm_eps) * w["layers.1.attn_norm.weight"]
        qkv = (x @ w["layers.1.attn.Wqkv.weight"].T).reshape(1, 48, 3, nh, hd).transpose(2, 0, 3, 1, 4)
        rot = lambda t: t * cos + np.concatenate([-t[..., hd // 2:], t[..., :hd // 2]], -1) * sin      # noqa: E731
        s = np.where(mc.window_mask(48, cfg.window)[None, None], rot(qkv[0]) @ rot(qkv[1]).transpose(0, 1, 3, 2) / math.sqrt(hd), -np.inf)
        a = np.exp(s - s.max(-1, keepdims=True))
        return ((a / a.sum(-1, keepdims=True)) @ qkv[2]).transpose(0, 2, 1, 3).reshape(1, 48, 64)
    moved = np.abs(attn(r) - attn(r2)).max(-1)[0] > 0
    assert np.flatnonzero(moved).tolist() == list(range(12, 29))


def test_wi_interleave_puts_input_and_gate_where_the_header_says():
    from rag._encoder import interleave_wi, split_gate_up
    text = open(os.path.join(ROOT, "include", "crs_encoder.h")).read()
    assert "rows [0, F) are the activated half" in text and "rows [F, 2F) the linear half" in text
    f, h = 96, 8
    wi = np.arange(2 * f * h, dtype=np.float32).reshape(2 * f, h)
    w = interleave_wi(wi)
    assert w.shape == (2 * f, h) and w.flags["C_CONTIGUOUS"]
    for j in range(f):                                          # the kernels' index formula: gelu acts on column gate_col(j)
        assert np.array_equal(w[gt.gate_col(j)], wi[j]) and np.array_equal(w[gt.gate_col(j) + 16], wi[f + j])
    act, lin = split_gate_up(w)
    assert np.array_equal(act, wi[:f]) and np.array_equal(lin, wi[f:])
    assert np.array_equal(interleave_wi(wi[:, 0]), w[:, 0])     # 1-d: the bias
    with pytest.raises(ValueError):
        interleave_wi(wi[:-1])


# ---- the loader ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("biases", [False, True])
def test_both_name_dialects_load_to_identical_internal_weights(tmp_path, biases):
    from rag.embedding import _load_local_dir
    from rag.tokenizer import BpeTokenizer
    cfg = mc.CFG_A
    w = mc.make_weights(cfg, 41, biases=biases)
    over = {"norm_bias": biases, "attention_bias": biases, "mlp_bias": biases}
    bare = _load_local_dir(mc.write_modernbert_dir(str(tmp_path / "bare"), cfg, w, cfg_over=over, max_seq=48))
    pref = _load_local_dir(mc.write_modernbert_dir(str(tmp_path / "pref"), cfg, w, prefix="model.", cfg_over=over, max_seq=48))
    assert bare[0] == pref[0]
    s = bare[0]
    assert (s.vocab_size, s.hidden, s.layers, s.heads, s.ffn, s.max_pos, s.max_seq) == (300, 64, 4, 4, 128, 256, 48)
    assert (s.prenorm, s.gelu_gated, s.gated, s.window, s.global_every, s.rotary_theta, s.local_theta) == (True, True, False, 8, 3, 160000.0, 10000.0)
    assert (s.ln_eps, s.pooling, s.rel_buckets, s.pos_offset) == (1e-5, "mean", 0, 0)
    assert sorted(bare[1]) == sorted(pref[1]) == sorted(w)
    for k, v in w.items():
        assert np.array_equal(bare[1][k], v) and np.array_equal(pref[1][k], v), k
    assert "layers.0.attn_norm.weight" not in w
    assert isinstance(bare[2], BpeTokenizer) and (bare[2].cls_id, bare[2].sep_id, bare[2].pad_id) == (mc.CLS_ID, mc.SEP_ID, mc.PAD_ID)
    # the older config keys: global_attn_every_n_layers and the two thetas, max_seq up to max_position_embeddings
    old = _load_local_dir(mc.write_modernbert_dir(str(tmp_path / "old"), cfg, w, max_seq=256, drop_keys=("layer_types", "rope_parameters"),
                                                  cfg_over={**over, "global_attn_every_n_layers": 3, "global_rope_theta": 160000.0,
                                                            "local_rope_theta": 10000.0}))
    assert old[0] == type(s)(**{**s.__dict__, "max_seq": 256})
    cls = _load_local_dir(mc.write_modernbert_dir(str(tmp_path / "cls"), cfg, w, cfg_over=over, pooling="cls"))
    assert cls[0].pooling == "cls"


REFUSED = [
    ({"hidden_activation": "silu"}, "hidden_activation"),
    ({"norm_bias": True}, "norm_bias"), ({"attention_bias": True}, "attention_bias"), ({"mlp_bias": True}, "mlp_bias"),
    ({"rope_parameters": {"full_attention": {"rope_type": "yarn", "rope_theta": 160000.0, "factor": 4.0},
                          "sliding_attention": {"rope_type": "default", "rope_theta": 10000.0}}}, "rope scaling"),
    ({"rope_parameters": {"full_attention": {"rope_type": "default", "rope_theta": 160000.0},
                          "sliding_attention": {"rope_type": "default", "rope_theta": 10000.0, "factor": 2.0}}}, "rope scaling"),
    ({"layer_types": ["full_attention", "sliding_attention", "full_attention", "full_attention"]}, "not periodic"),
    ({"layer_types": ["sliding_attention", "full_attention", "sliding_attention", "full_attention"]}, "not periodic"),
    ({"architectures": ["ModernBertForSequenceClassification"]}, "ModernBertForSequenceClassification"),
    ({"architectures": ["ModernBertForMaskedLM"]}, "ModernBertForMaskedLM"),
    ({"local_attention": 1}, "local_attention"),
]


@pytest.mark.parametrize("over,word", REFUSED, ids=[w for _, w in REFUSED])
def test_refused_options_are_named(tmp_path, over, word):
    from rag.embedding import _load_local_dir
    d = mc.write_modernbert_dir(str(tmp_path), mc.CFG_A, mc.make_weights(mc.CFG_A, 42), cfg_over=over)
    with pytest.raises(NotImplementedError, match=word):
        _load_local_dir(d)


def test_old_style_rope_scaling_and_head_tensors_are_refused(tmp_path):
    from rag.embedding import _load_local_dir
    w = mc.make_weights(mc.CFG_A, 43)
    d = mc.write_modernbert_dir(str(tmp_path / "s"), mc.CFG_A, w, drop_keys=("rope_parameters",), cfg_over={"rope_scaling": {"type": "linear", "factor": 2.0}})
    with pytest.raises(NotImplementedError, match="rope scaling"):
        _load_local_dir(d)
    w["head.dense.weight"] = np.zeros((64, 64), dtype=np.float32)
    d = mc.write_modernbert_dir(str(tmp_path / "h"), mc.CFG_A, w, prefix="model.")
    with pytest.raises(NotImplementedError, match="task head"):
        _load_local_dir(d)


def test_other_loaders_keep_refusing_the_model_type(tmp_path):
    """The re-ranker, ColBERT, SPLADE and BERTScore loaders read BERT-family directories only."""
    d = mc.write_modernbert_dir(str(tmp_path), mc.CFG_A, mc.make_weights(mc.CFG_A, 44))
    from rag.bertscore import load_hf_dir
    from rag.late_interaction import load_late_interaction_dir
    from rag.reranking import load_cross_encoder_dir
    from rag.sparse import load_sparse_dir
    for load in (load_cross_encoder_dir, load_late_interaction_dir, load_sparse_dir, load_hf_dir):
        with pytest.raises(NotImplementedError, match="model_type 'modernbert' is not supported"):
            load(d)


# ---- the tokeniser ---------------------------------------------------------------------------------------------------------------
def test_tokeniser_ids_equal_the_fixture(tmp_path):
    from rag.tokenizer import BpeTokenizer, tokenizer_from_model_dir
    cases = json.load(open(mc.TOKENIZER_CASES, encoding="utf-8"))
    assert len(cases["texts"]) >= 12
    d = mc.write_modernbert_dir(str(tmp_path), mc.CFG_A, mc.make_weights(mc.CFG_A, 45))
    tok = tokenizer_from_model_dir(d)
    assert isinstance(tok, BpeTokenizer)
    n = cases["max_seq"]
    rows = tok.encode_batch([t.strip() for t in cases["texts"]], n)
    assert rows == cases["ids"] == [tok.encode(t.strip(), n) for t in cases["texts"]]
    assert all(r[0] == mc.CLS_ID and r[-1] == mc.SEP_ID and len(r) <= n for r in rows)
    assert max(len(r) for r in rows) == n and rows[3] == [mc.CLS_ID, mc.SEP_ID]            # a truncated text, and the empty one
    assert tok.encode(cases["texts"][-1].strip(), 10) == rows[-1][:9] + [mc.SEP_ID]         # cut to max_seq, [SEP] kept
    assert tok.encode_body("the quick brown fox") == rows[0][1:-1]
    assert max(max(r) for r in rows) < mc.CFG_A.vocab_size


def test_without_the_tokenizers_library_the_error_says_so(tmp_path, monkeypatch):
    import sys
    from rag.tokenizer import tokenizer_from_model_dir
    d = mc.write_modernbert_dir(str(tmp_path), mc.CFG_A, mc.make_weights(mc.CFG_A, 46))
    monkeypatch.setitem(sys.modules, "tokenizers", None)        # `import tokenizers` now raises ImportError
    with pytest.raises(ImportError, match="byte-level BPE tokenizer.json: loading it needs the `tokenizers` library"):
        tokenizer_from_model_dir(d)


def test_golden_records_what_made_it(golden):
    assert str(golden["meta.transformers_version"]) and "eager_attention_forward" in str(golden["meta.patched"])
    assert "unpadded" in str(golden["meta.patched"])


# ---- planner, symbols ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mb_plan") / "enc_plan_table")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tools", "enc_plan_table.cpp"),
                    os.path.join(CSRC, "enc_plan.cpp")], check=True, timeout=300)

    def run(lines, env=None):
        e = {k: v for k, v in os.environ.items() if not k.startswith("CRS_")}
        e.update(env or {})
        r = subprocess.run([exe, "256"], input="".join(" ".join(map(str, c)) + "\n" for c in lines), env=e, capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 0, r.stderr
        return [ln.split("\t") for ln in r.stdout.splitlines()]
    return run


FLAGS = 2 | 8 | 16


def test_planner_lines_for_tiny_and_base_shapes(table):
    tiny, base512, base8k = table([("fwdw", 64, 4, 128, FLAGS, 3, 144, 0, 0, 8), ("fwdw", 768, 12, 1152, FLAGS, 64, 512, 0, 0, 64),
                                   ("fwdw", 768, 12, 1152, FLAGS, 8, 8192, 0, 0, 64)])
    assert tiny[1].split(";")[:-1] == [
        "embed_ln_kernel<1, false> grid=108x1x1 wg=256x1x1 lds=0", "gemm_f16_kernel<0> grid=8x1x1 wg=256x1x1 lds=0",
        "rope_qk_kernel<16> grid=14x1x1 wg=256x1x1 lds=0", "attention_seq_kernel<16, 256, 4> grid=12x1x1 wg=256x1x1 lds=18560",
        "attention_window_kernel<16> grid=3x4x3 wg=256x1x1 lds=0", "gemm_f16_kernel<2> grid=4x1x1 wg=256x1x1 lds=0",
        "add_layernorm_kernel<1, 1> grid=108x1x1 wg=256x1x1 lds=0", "gemm_f16_kernel<5> grid=8x1x1 wg=256x1x1 lds=0",
        "gemm_panel_kernel<3, 64> grid=1x7x1 wg=512x1x1 lds=32768", "add_layernorm_kernel<1, 1> grid=108x1x1 wg=256x1x1 lds=0",
        "pool_kernel grid=3x1x1 wg=256x1x1 lds=0"]
    lines = base512[1].split(";")[:-1]
    assert lines[3] == "attention_seq32_kernel<64, 512, 8, 2> grid=768x1x1 wg=512x1x1 lds=140288"
    assert lines[4] == "attention_window_kernel<64> grid=8x12x64 wg=256x1x1 lds=0"
    assert lines[6] == lines[9] == "add_layernorm2_kernel<6, 1> grid=8192x1x1 wg=256x1x1 lds=0"
    assert lines[7] == "gemm8_kernel<5, true, 0> grid=256x1x1 wg=512x1x1 lds=149504"
    lines = base8k[1].split(";")[:-1]
    assert lines[3] == "attention_kernel<64, false> grid=128x12x8 wg=256x1x1 lds=0"          # past the whole-sequence kernels' 512
    assert lines[4] == "attention_window_kernel<64> grid=128x12x8 wg=256x1x1 lds=0"


def test_prenorm_never_selects_the_fused_kernels_and_changes_no_other_plan(table):
    """Over the shapes where a post-norm model takes qkv_attn_kernel (short sequences, hidden <= 384) or gemm_rowln2_kernel (hidden
    384 past 4096 tokens): the pre-norm plan has neither, whatever the knobs; and the same shapes without the new flags print what
    they printed before (the post-norm lines carry no new name)."""
    shapes = [(384, 12, 1536, b, s) for b, s in ((8, 16), (64, 32), (64, 64), (256, 16), (128, 64), (512, 256))] + \
             [(256, 8, 1024, 16, 64), (128, 2, 512, 4, 32), (768, 12, 1152, 512, 16)]
    for env in (None, {"CRS_ENC_BIGLN": "1", "CRS_ENC_QKVATTN": "1"}, {"CRS_GEMM8": "0"}, {"CRS_SPLITK_MAX_TOKENS": "65536"}):
        pre = table([("fwdw", h, nh, f, FLAGS, b, s, 0, 0, 64) for h, nh, f, b, s in shapes], env)
        post = table([("fwd", h, nh, f, 0, b, s, 0, 0) for h, nh, f, b, s in shapes], env)
        for (fields, text), (_, ptext) in zip(pre, post):
            assert "qkv_attn_kernel" not in text and "rowln2" not in text and "out_rowln2=0 down_rowln2=0" in fields
            assert "attn=Fused" not in fields and ";layernorm" not in text
            assert text.count("add_layernorm") == 2 and "attention_window_kernel" in text
            assert "add_layernorm" not in ptext and "window" not in ptext and "<5" not in ptext
        assert any("qkv_attn_kernel" in t for _, t in post) and any("rowln2" in t for _, t in post)


def test_mode_5_routes_where_mode_4_does_and_never_to_big_or_stream(table):
    shapes = [(m, n, k) for m in (1, 65, 512, 2048, 4096, 16384, 32768) for n in (128, 384, 2304, 3072) for k in (64, 384, 768, 1024)]
    for env in (None, {"CRS_GEMM8": "0"}, {"CRS_GEMM_BIG_MIN_WGS": "1"}, {"CRS_GEMM8": "0", "CRS_GEMM_BIG_MIN_WGS": "1"}):
        for route in (0, 1):
            m5 = table([("route", m, n, k, 5, route, 0) for m, n, k in shapes], env)
            m4 = table([("route", m, n, k, 4, route, 0) for m, n, k in shapes], env)
            m1 = table([("route", m, n, k, 1, route, 0) for m, n, k in shapes], env)
            for (f5, t5), (f4, t4) in zip(m5, m4):
                assert f5 == f4 and t5 == re.sub(r"<4([,>])", r"<5\1", t4)
                assert "gemm_big" not in t5 and "gemm_stream" not in t5
            if route == 0:
                assert any("gemm_big" in t or "gemm_stream" in t for _, t in m1)           # the shapes do reach those families in mode 1


def test_new_entry_points_are_declared_exported_and_bound():
    from rag import _native as nat
    import rag._encoder as enc
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crs_encoder.h")).read(), flags=re.S)
    lib = nat.load()
    names = ("crs_encoder_forward_prenorm", "crs_encoder_forward_queries_prenorm", "crs_encoder_prenorm_plan_describe",
             "crs_attention_window_f16", "crs_attention_window_plan_describe", "crs_add_layernorm_f32")
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in names:
        assert re.search(r"\bint %s\s*\(" % name, text), f"{name} is not declared"
        assert hasattr(lib, name) and name in nat.exported_symbols()
        assert name in doc, f"{name} not documented in INTEGRATION.md"
    assert re.search(r"#define CRS_ENC_PRENORM 8\b", text) and re.search(r"#define CRS_ENC_GATED_GELU 16\b", text)
    assert (enc.ENC_PRENORM, enc.ENC_GATED_GELU) == (8, 16)
    assert re.search(r"const float\* rope_global_dev;[^}]*rope_local_dev;[^}]*positions;[^}]*window;[^}]*global_every;[^}]*final_ln_g;", text)
    assert lib.crs_abi_version() == 3
    assert hasattr(nat.ops(), "encoder_forward_prenorm")
    s = enc.ModelShape(1000, 64, 2, 4, 256, 64)
    assert (s.prenorm, s.window, s.global_every, s.local_theta, s.gelu_gated) == (False, 0, 1, 0.0, False)
    # describes need no device
    assert enc.attention_window_plan_describe(2, 200, 128, 2, 8) == "attention_window_kernel<64> grid=4x2x2 wg=256x1x1 lds=0\n"
    assert enc.row_plan_describe(enc.ROW_ADD_LAYERNORM, 13, 768, 4) == "add_layernorm2_kernel<6, 4> grid=4x1x1 wg=256x1x1 lds=0\n"
    for bad in (lambda: enc.attention_window_plan_describe(2, 200, 128, 2, 0), lambda: enc.row_plan_describe(4, 13, 768, 5),
                lambda: enc.attention_window_plan_describe(2, 200, 128, 16, 8)):
        with pytest.raises(nat.NativeError):
            bad()
    from rag.embedding import _KNOWN
    assert _KNOWN["modernbert-base"]["ffn"] == 1152 and _KNOWN["modernbert-base"]["layers"] == 22 and _KNOWN["modernbert-base"]["window"] == 64


# ---- the kernels' fp32 emulations inside their bounds, planted faults far outside ------------------------------------------------
WIN_CPU = [(16, 4, 8, 144), (64, 2, 8, 80), (32, 3, 1, 80), (16, 4, 64, 200), (64, 2, 200, 144)]


@pytest.mark.parametrize("hd,heads,window,seq", WIN_CPU)
def test_window_emulation_stays_inside_the_bound_and_faults_leave_it(hd, heads, window, seq):
    lens = [seq, 5, (seq * 5) // 8]
    batch = len(lens)
    qkv = ar.make_inputs(batch, seq, heads, hd, lens, seed=hd + window + seq, peaked=True)
    ref, bound = aw.ref_and_bound(qkv, lens, batch, seq, heads, hd, window)
    out = aw.emulate(qkv, lens, batch, seq, heads, hd, window)
    r, finite = aw.ratio_real(out, ref, bound, lens, batch, seq)
    print(hd, window, seq, "ratio", r)
    assert finite and r <= 1.0
    no_key = np.arange(seq) >= 5 + window
    assert (out[seq:2 * seq][no_key] == 0).all()
    if window >= seq:                                   # the full-attention reference and bound hold it too
        fr, fb, _ = ar.ref_and_bound(qkv, lens, batch, seq, heads, hd)
        assert ar.ratio(out, fr, fb) <= 1.0 and ar.ratio(ar.emulate(qkv, lens, batch, seq, heads, hd), fr, fb) <= 1.0
        return
    for fault in aw.WIN_FAULTS:
        if fault == "sentinel_not_wiped" and window >= 64:
            continue                                    # no query's first visited block lies wholly outside such a window
        rf, _ = aw.ratio_real(aw.emulate(qkv, lens, batch, seq, heads, hd, window, fault=fault), ref, bound, lens, batch, seq)
        print("  ", fault, rf)
        assert rf > WIDE, fault


def _emulate_add_ln(y, bias, res, g, b, eps, fault=None):
    """add_layernorm*_kernel in fp32: (r32, n32, x16).  fault residual_not_written: r32 keeps the old residual."""
    a = y[0].copy()
    for s in range(1, y.shape[0]):
        a = a + y[s]
    if bias is not None:
        a = a + bias[None, :]
    if res is not None:
        a = a + res
    a = a.astype(np.float32)
    n32, x16 = rr.emulate_ln_store(a, g, b if b is not None else np.zeros_like(g), eps, None if fault == "residual_not_written" else fault)
    return (res.copy() if fault == "residual_not_written" else a), n32, x16


@pytest.mark.parametrize("hidden,nsplit", [(64, 1), (64, 16), (384, 2), (768, 4), (1024, 6), (320, 3)])
def test_add_layernorm_emulation_stays_inside_the_bounds_and_faults_leave_them(hidden, nsplit):
    g = torch.Generator().manual_seed(hidden + nsplit)
    y = torch.randn((nsplit, 13, hidden), generator=g) * 0.7
    res = torch.randn((13, hidden), generator=g) * 1.3
    bias = torch.randn(hidden, generator=g) * 0.4
    gain = 1.0 + 0.2 * torch.randn(hidden, generator=g)
    for beta in (0.3 * torch.randn(hidden, generator=g), None):
        v, e = rr.sum_ref_and_err(rr.ln_terms(y, bias, res))
        ref, b32, b16, frac = rr.layernorm_ref_and_bound(y, bias, res, gain, beta if beta is not None else torch.zeros(hidden), 1e-5)
        assert frac < rr.SECOND_ORDER_LIMIT
        args = (y.numpy(), bias.numpy(), res.numpy(), gain.numpy(), None if beta is None else beta.numpy(), 1e-5)
        r32, n32, x16 = _emulate_add_ln(*args)
        assert rr.ratio(torch.from_numpy(r32), v, e + rr.TINY) <= 1.0
        assert rr.ratio(torch.from_numpy(n32), ref, b32) <= 1.0 and rr.ratio(torch.from_numpy(x16), ref, b16) <= 1.0
        r32f, _, _ = _emulate_add_ln(*args, fault="residual_not_written")
        assert rr.ratio(torch.from_numpy(r32f), v, e + rr.TINY) > 1e4
        # a skipped bias / slab shifts r32 and the normalised row alike
        for fault in ("bias_skipped", "last_slab_dropped") if nsplit > 1 else ("bias_skipped",):
            yy = args[0][:-1] if fault == "last_slab_dropped" else args[0]
            r32f, n32f, _ = _emulate_add_ln(yy, None if fault == "bias_skipped" else args[1], *args[2:])
            assert rr.ratio(torch.from_numpy(r32f), v, e + rr.TINY) > 1e4 and rr.ratio(torch.from_numpy(n32f), ref, b32) > WIDE, fault


@pytest.mark.parametrize("m,f,k", [(65, 64, 64), (33, 192, 384), (7, 64, 768)])
def test_gelu_gated_emulation_stays_inside_the_bound_and_silu_leaves_it(m, f, k):
    a, w, bias = gt.make_inputs(m, f, k)
    for b in (bias, None):
        ref, bound = gg.ref_and_bound(a, w, b)
        r = gr.ratio(gg.emulate(a, w, b), ref, bound)
        print(m, f, k, "ratio", r)
        assert r <= 1.0
        for fault in gg.FAULTS:
            rf = gr.ratio(gg.emulate(a, w, b, fault=fault), ref, bound)
            print("  ", fault, rf)
            assert rf > WIDE, fault
        assert gr.ratio(gt.emulate(a, w, b), ref, bound) > WIDE          # mode 4's own emulation: SiLU in place of GELU
