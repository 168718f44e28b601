"""GPU parity of the rotary, gated encoder family (nomic-embed-text): the forward against transformers.NomicBertModel in fp64
(tests/golden/encoder_nomic.npz, tools/make_nomic_golden.py) and against the fp64 restatement at the key-block and position
edges, rope_qk_kernel and GEMM mode 4 on their own under derived bounds, the CRS_EINVAL cases, the small-LDS selection, the
graph-captured query forward of the retrieval engine with task prefixes, and device tokenisation with a prefix.
Tolerances of the forward: tests/test_mpnet_gpu.py's (the project's own encoder bounds)."""
import re

import numpy as np
import pytest

import _gated_ref as gt
import _gemm_ref as gr
import _nomic_cases as nc

pytestmark = pytest.mark.gpu


def _cos(a, b):
    return (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


@pytest.fixture(scope="module")
def golden():
    return np.load(nc.GOLDEN)


def _nomic_encoder(cfg, seed, cuda, **over):
    from dataclasses import replace
    from rag._encoder import HipEncoder
    shape = replace(nc.model_shape(cfg), **over)
    return HipEncoder(shape, nc.make_weights(cfg, seed), device=cuda)


def _assert_forward_bounds(figures):
    assert figures["hidden"] < 3e-2
    assert figures["mean_cos"] < 2e-4 and figures["cls_cos"] < 2e-4
    assert figures["mean_abs"] < 3e-3 and figures["cls_abs"] < 3e-3
    if "pair" in figures:
        assert figures["pair"] < 1e-3


def _golden_figures(enc, z, key, cfg, **kw):
    import torch
    ids, mask = z[key + ".ids"], z[key + ".mask"].astype(np.int32)
    lens = mask.sum(1).astype(np.int32)
    mean, hidden = enc.forward(ids, lens, return_hidden=True, **kw)
    enc.desc.pooling = 1
    cls = enc.forward(ids, lens, **kw)
    enc.desc.pooling = 0
    torch.cuda.synchronize()
    mean, cls = mean.cpu().numpy(), cls.cpu().numpy()
    hid = hidden.cpu().numpy().reshape(-1, cfg.hidden)[z[key + ".rows"]]
    return dict(hidden=np.abs(hid - z[key + ".hidden"]).max(), mean_cos=(1.0 - _cos(mean, z[key + ".mean_norm"])).max(),
                cls_cos=(1.0 - _cos(cls, z[key + ".cls_norm"])).max(), mean_abs=np.abs(mean - z[key + ".mean_norm"]).max(),
                cls_abs=np.abs(cls - z[key + ".cls_norm"]).max(),
                pair=np.abs(mean @ mean.T - z[key + ".mean_norm"] @ z[key + ".mean_norm"].T).max()), (mean, hidden)


@pytest.mark.parametrize("key", [c[0] for c in nc.CASES])
def test_forward_matches_transformers_nomic(cuda, golden, key):
    _, cfg, seed, batch, seq = next(c for c in nc.CASES if c[0] == key)
    assert int(golden[key + ".seed"]) == seed and golden[key + ".ids"].shape == (batch, seq)
    enc = _nomic_encoder(cfg, seed, cuda)
    assert enc.rope_table is not None and tuple(enc.rope_table.shape) == (cfg.max_seq, cfg.hidden // cfg.heads)
    assert enc.desc.flags == 6 and enc.rel_bias is None
    figures, _ = _golden_figures(enc, golden, key, cfg)
    print(key, {k: float(v) for k, v in figures.items()})
    _assert_forward_bounds(figures)


# (config, seq): TINY at 1 and 64: a single position (the identity rotation) / exactly one key block.  MID at 65 (a second key
# block of one key), 129 and 256 (its max_seq: a whole number of key blocks, the whole rope table).  BASE at 65, and at 513: one
# position past BERT's table and past the whole-sequence attention kernels' limit.
EDGES = [(nc.TINY, 1), (nc.TINY, 64), (nc.MID, 65), (nc.MID, 129), (nc.MID, 256), (nc.BASE, 65), (nc.BASE, 513)]


@pytest.mark.parametrize("cfg,seq", EDGES, ids=[f"{c.name}-{s}" for c, s in EDGES])
def test_key_block_and_position_edges_match_fp64(cuda, cfg, seq):
    """The forward against _nomic_cases.encode_ref (fp64, exact cos / sin): batch 2, one full row and one row of a single token."""
    import torch
    from _encoder_cases import pool
    seed = 400 + seq
    w = nc.make_weights(cfg, seed)
    enc = _nomic_encoder(cfg, seed, cuda)
    ids = np.random.default_rng(seed + 1).integers(103, cfg.vocab_size, size=(2, seq)).astype(np.int32)
    lens = np.array([seq, 1], dtype=np.int32)
    mask = (np.arange(seq)[None, :] < lens[:, None]).astype(np.int32)
    ids[:, 0], ids[1, 1:] = nc.CLS_ID, nc.PAD_ID
    if seq > 1:
        ids[0, seq - 1] = nc.SEP_ID
    ref_h = nc.encode_ref(ids, mask, w, cfg)
    mean, hidden = enc.forward(ids, lens, return_hidden=True)
    enc.desc.pooling = 1
    cls = enc.forward(ids, lens)
    torch.cuda.synchronize()
    valid = mask.astype(bool)
    figures = dict(hidden=np.abs(hidden.cpu().numpy()[valid] - ref_h[valid]).max())
    for name, got in (("mean", mean.cpu().numpy()), ("cls", cls.cpu().numpy())):
        ref = pool(ref_h, mask, name, True)
        figures[name + "_cos"], figures[name + "_abs"] = (1.0 - _cos(got, ref)).max(), np.abs(got - ref).max()
    print(cfg.name, seq, {k: float(v) for k, v in figures.items()})
    _assert_forward_bounds(figures)


@pytest.mark.parametrize("which", ["all", "qkv_only", "mlp_only"])
def test_checkpoint_biases_are_passed(cuda, which):
    """A checkpoint that enables biases: the concatenated q / k / v bias, the interleaved gate / up bias (mode 4's b[g], b[g + 16])
    and the plain ones reach the kernels; where a bias is missing its zero vector (b_up: NULL) stands in.  TINY (FFN-up on the tiled
    kernel) and MID (the panel kernel) against encode_ref with the same biases; they are O(0.3), so a dropped or misplaced one fails."""
    import torch
    for cfg, seed, batch, seq in ((nc.TINY, 501, 3, 24), (nc.MID, 502, 2, 40)):
        w = nc.make_weights(cfg, seed)
        rng = np.random.default_rng(seed)
        for i in range(cfg.layers):
            p = f"layers.{i}."
            names = []
            if which in ("all", "qkv_only"):
                names += [(p + f"self_attn.{n}_proj.bias", cfg.hidden) for n in "qkv"]
            if which in ("all", "mlp_only"):
                names += [(p + "mlp.gate_proj.bias", cfg.ffn), (p + "mlp.up_proj.bias", cfg.ffn), (p + "mlp.down_proj.bias", cfg.hidden)]
            if which == "all":
                names += [(p + "self_attn.o_proj.bias", cfg.hidden)]
            for name, n in names:
                w[name] = (0.3 * rng.standard_normal(n)).astype(np.float32)
        from rag._encoder import HipEncoder
        enc = HipEncoder(nc.model_shape(cfg), w, device=cuda)
        ids, mask = nc.synth_tokens(cfg, batch, seq, seed + 1)
        lens = mask.sum(1).astype(np.int32)
        ref_h = nc.encode_ref(ids, mask, w, cfg)
        plain_h = nc.encode_ref(ids, mask, nc.make_weights(cfg, seed), cfg)
        mean, hidden = enc.forward(ids, lens, return_hidden=True)
        torch.cuda.synchronize()
        valid = mask.astype(bool)
        m = (ref_h * mask[..., None]).sum(1) / mask.sum(1, keepdims=True)
        m /= np.linalg.norm(m, axis=1, keepdims=True)
        got = mean.cpu().numpy()
        figures = dict(hidden=np.abs(hidden.cpu().numpy()[valid] - ref_h[valid]).max(), cos=(1.0 - _cos(got, m)).max(), abs=np.abs(got - m).max(),
                       moved=np.abs(plain_h[valid] - ref_h[valid]).max())
        print(cfg.name, which, {k: float(v) for k, v in figures.items()})
        assert figures["moved"] > 0.1                           # the biases matter: 3x the hidden-state bound at least
        assert figures["hidden"] < 3e-2 and figures["cos"] < 2e-4 and figures["abs"] < 3e-3


# ---- rope_qk_kernel on its own -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd,heads", [(16, 4), (32, 12), (64, 3)])
@pytest.mark.parametrize("seq", [1, 5, 64, 65, 600])
@pytest.mark.parametrize("batch", [1, 3])
def test_rope_kernel_alone_against_fp64(cuda, hd, heads, seq, batch):
    """crs_rope_qk_f16 on a canary-framed [T, 3H] buffer against the fp64 rotation of its fp16 inputs with EXACT cos / sin.
    Bound, per output t' = x c -+ y s (x, y fp16 values, exact in fp32; u = 2^-24): the table entries are fp64 values rounded
    once (u relative each), each product rounds once (u) and the sum once more (u of at most |x c| + |y s|) -- a fused
    multiply-add only removes a rounding -- so the fp32 value errs by at most e = 4 u (|x c| + |y s|); then one rounding to
    fp16: half an fp16 ulp of (|ref| + e).  V and the frame keep their bits."""
    import torch
    from rag._encoder import rope_qk_f16, rope_table
    h, t = hd * heads, batch * seq
    g = torch.Generator().manual_seed(hd * 1000 + seq * 7 + batch)
    frame = 2                                                   # rows of canary before and after
    buf = (torch.randn((t + 2 * frame, 3 * h), generator=g) * 1.5).half()
    buf[:frame], buf[-frame:] = 77.0, -77.0
    positions = seq + 3                                         # a table longer than the sequence: rows past seq are not used
    table = torch.from_numpy(rope_table(positions, hd, nc.THETA))
    dev = buf.to(cuda)
    rope_qk_f16(dev[frame:frame + t], table.to(cuda), batch, seq, heads)
    torch.cuda.synchronize()
    out = dev.cpu()
    assert torch.equal(out[:frame], buf[:frame]) and torch.equal(out[-frame:], buf[-frame:])
    assert torch.equal(out[frame:-frame, 2 * h:], buf[frame:-frame, 2 * h:])                # V
    x = buf[frame:-frame, :2 * h].double().view(batch, seq, 2 * heads, hd)
    c, s = (torch.from_numpy(a)[:seq] for a in nc.rope_cos_sin(positions, hd))
    c, s = c[None, :, None, :], s[None, :, None, :]
    lo, hi = x[..., :hd // 2], x[..., hd // 2:]
    ref = torch.cat([lo * c - hi * s, hi * c + lo * s], dim=-1)
    mag = torch.cat([(lo * c).abs() + (hi * s).abs(), (hi * c).abs() + (lo * s).abs()], dim=-1)
    e = 4.0 * gr.U * mag
    bound = e + gr.half_ulp16(ref.abs() + e)
    got = out[frame:-frame, :2 * h].double().view(batch, seq, 2 * heads, hd)
    r = ((got - ref).abs() / bound).max().item()
    print(hd, seq, batch, "ratio", r)
    assert r <= 1.0
    if seq > 1:                                                 # (position 0 is the identity)
        assert not torch.equal(out[frame + 1:frame + 2, :2 * h], buf[frame + 1:frame + 2, :2 * h])
    assert torch.equal(out[frame::seq][:batch, :2 * h], buf[frame::seq][:batch, :2 * h])    # position 0 of every sequence: bit-identical


# ---- GEMM mode 4 on its own, per family ----------------------------------------------------------------------------------------
TILED = [(0, 0, m, f, k) for m in (1, 65, 200) for f in (64, 192, 1536) for k in (64, 384, 768)]
# the panel kernel stages K in chunks of 128 / 256 / 384: K = 64 is not one of its shapes.  flags 1: the small-LDS form
PANEL = [(1, fl, m, f, k) for fl in (0, 1) for m in (1, 65, 200) for f in (64, 192, 1536) for k in (384, 768)]
# the row counts at which modes 0 / 1 leave the tiled kernel for the row-streaming kernels (512 rows): mode 4 stays
LARGE = [(0, 0, 512, 1536, 768), (0, 0, 2048, 192, 384)]
# the 256 x 256 phase-scheduled kernel at the smallest row counts it accepts (128 tiles of [M, 2F]; K >= 256 in whole 128-column
# steps; 2F = 128 has no form), one workgroup per item -- and, at 5632 rows (264 items > 256 CUs), its persistent form
GEMM8 = [(0, 0, 2816, 1536, 384), (0, 0, 2816, 1536, 768), (0, 0, 16384, 192, 384), (0, 0, 5632, 1536, 384)]


@pytest.mark.parametrize("route,flags,m,f,k", TILED + PANEL + LARGE + GEMM8)
def test_gated_gemm_alone_under_the_derived_bound(cuda, route, flags, m, f, k):
    import torch
    from rag._encoder import gemm_f16_routed, gemm_plan_describe
    line, slabs = gemm_plan_describe(m, 2 * f, k, 4, route, flags)
    assert slabs == 1
    if (route, flags, m, f, k) in GEMM8:
        cus = torch.cuda.get_device_properties(cuda).multi_processor_count
        items = (m // 256) * (2 * f // 256)
        assert line.startswith(f"gemm8_kernel<4, {'true' if items > cus else 'false'}, 0> "), line
    elif route == 0:
        assert line.startswith("gemm_f16_kernel<4> ")
    else:
        assert re.match(r"gemm_panel_kernel<4, (64|128)> ", line)
        if flags:
            assert int(re.search(r"lds=(\d+)", line).group(1)) <= 48 * 1024
    a, w, bias = gt.make_inputs(m, f, k)
    ps = gr.products(a, w, 1)
    frame = 8                                                   # canary rows around the output
    for b in (bias, None):
        ref, bound = gt.gated_ref_and_bound(a, w, b, ps=ps)
        out = torch.full((m + 2 * frame, f), 7.0, dtype=torch.float16, device=cuda)
        gemm_f16_routed(a.to(cuda), w.to(cuda), None if b is None else b.to(cuda), None, out[frame:frame + m], 4, route, flags)
        torch.cuda.synchronize()
        got = out.cpu()
        assert (got[:frame] == 7.0).all() and (got[-frame:] == 7.0).all()
        r = gr.ratio(got[frame:-frame], ref, bound)
        print(line.split()[0], m, f, k, "bias" if b is not None else "no bias", "ratio", r)
        assert r <= 1.0


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_einval_cases_leave_the_outputs_untouched(cuda, golden):
    import torch
    from rag import _native as nat
    from rag._encoder import ModelShape, gemm_f16_routed, gemm_plan_describe, rope_qk_f16, rope_table
    cfg, seed = nc.TINY, 201
    enc = _nomic_encoder(cfg, seed, cuda, max_seq=16)            # a table of 16 positions
    assert tuple(enc.rope_table.shape) == (16, 16)
    ids, mask = nc.synth_tokens(cfg, 2, 24, 7)
    lens = mask.sum(1).astype(np.int32)
    out = torch.full((2, 64), 7.0, dtype=torch.float32, device=cuda)
    q16 = torch.full((2, nat.padded_dim(64)), 7.0, dtype=torch.float16, device=cuda)
    hid = torch.full((2, 24, 64), 7.0, dtype=torch.float32, device=cuda)

    def untouched():
        torch.cuda.synchronize()
        return (out == 7.0).all().item() and (q16 == 7.0).all().item() and (hid == 7.0).all().item()

    # positions < seq
    with pytest.raises(nat.NativeError, match=r"error -1: .*positions 16 .*seq 24"):
        enc.forward(ids, lens, out=out)
    with pytest.raises(nat.NativeError, match=r"error -1: .*positions 16"):
        enc.forward(ids, lens, out=out, q16_out=q16)
    assert untouched()
    assert torch.isfinite(enc.forward(ids[:, :16], np.minimum(lens, 16))).all().item()      # positions == seq is served
    # CRS_ENC_ROTARY without a table: through the entry points that carry none, and with the table taken away
    ws = torch.empty(enc.workspace_bytes(2, 16), dtype=torch.uint8, device=cuda)
    ids16 = torch.from_numpy(ids[:, :16].copy()).to(cuda)
    lens16 = torch.from_numpy(np.minimum(lens, 16)).to(cuda)
    for call in (lambda: nat.ops().encoder_forward_ex(ids16, lens16, enc._wlist, enc._desc_list, 1e-12, ws, out, None, 0, True, hid[:, :16].contiguous(), None),
                 lambda: nat.ops().encoder_forward(ids16, lens16, enc._wlist, enc._desc_list, 1e-12, ws, out, q16, 0, True, None),
                 lambda: nat.ops().encoder_forward_rope(ids16, lens16, enc._wlist, enc._desc_list, 1e-12, ws, out, None, 0, True, None, None, None)):
        with pytest.raises(nat.NativeError, match=r"error -1: .*CRS_ENC_ROTARY needs a rope table"), nat._translate():
            call()
    assert untouched()
    # CRS_ENC_ROTARY together with a relative-position bias
    bias = torch.zeros((4, 31), dtype=torch.float32, device=cuda)
    with pytest.raises(nat.NativeError, match=r"error -1: .*relative-position bias"), nat._translate():
        nat.ops().encoder_forward_rope(ids16, lens16, enc._wlist, enc._desc_list, 1e-12, ws, out, None, 0, True, None, bias, enc.rope_table)
    assert untouched()
    # CRS_ENC_GATED_SILU with ffn % 64 != 0 (the descriptor check)
    bad = enc._desc_list
    bad[4] = 96
    with pytest.raises(nat.NativeError, match=r"error -1: .*ffn must be a multiple of 64"), nat._translate():
        nat.ops().encoder_forward_rope(ids16, lens16, enc._wlist, bad, 1e-12, ws, out, None, 0, True, None, None, enc.rope_table)
    assert untouched()
    # mode 4 with odd N, and with N / 2 not a multiple of 32
    a = torch.zeros((8, 128), dtype=torch.float16, device=cuda)
    for n in (65, 96, 160):
        w = torch.zeros((n, 128), dtype=torch.float16, device=cuda)
        o = torch.full((8, n), 7.0, dtype=torch.float16, device=cuda)
        for route in (0, 1):
            with pytest.raises(nat.NativeError, match=r"error -1: .*mode 4"):
                gemm_f16_routed(a, w, None, None, o, 4, route, 0)
            with pytest.raises(nat.NativeError, match=r"error -1: .*mode 4"):
                gemm_plan_describe(8, n, 128, 4, route, 0)
        torch.cuda.synchronize()
        assert (o == 7.0).all().item()
    with pytest.raises(nat.NativeError, match=r"error -1"):                                   # the split-K route has no mode 4
        gemm_plan_describe(2048, 512, 1024, 4, 2, 0)
    # the rope step on its own: positions < seq, a head_dim it has no form for
    qkv = torch.full((10, 3 * 64), 7.0, dtype=torch.float16, device=cuda)
    with pytest.raises(nat.NativeError, match=r"error -1: .*positions"):
        rope_qk_f16(qkv, torch.from_numpy(rope_table(4, 16, 1000.0)).to(cuda), 2, 5, 4)
    with pytest.raises(nat.NativeError, match=r"error -1: .*head_dim"):
        rope_qk_f16(qkv, torch.from_numpy(rope_table(8, 8, 1000.0)).to(cuda), 2, 5, 8)
    torch.cuda.synchronize()
    assert (qkv == 7.0).all().item()
    # a shape that is rotary but not gated has no loader
    with pytest.raises(NotImplementedError):
        _nomic_encoder(cfg, seed, cuda, gated=False)


# ---- the small-LDS selection ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["tiny_4x24", "mid_3x80", "base_2x16", "base_1x150"])
def test_small_lds_selection_stays_within_the_bounds(cuda, golden, key):
    import torch
    from rag import _native as nat
    from rag._encoder import EncoderDesc
    _, cfg, seed, batch, seq = next(c for c in nc.CASES if c[0] == key)
    enc = _nomic_encoder(cfg, seed, cuda)
    figures, (a, ha) = _golden_figures(enc, golden, key, cfg, small_lds=True)
    print(key, "small_lds", {k: float(v) for k, v in figures.items()})
    _assert_forward_bounds(figures)
    d = enc.desc
    small = EncoderDesc(d.vocab_size, d.hidden, d.layers, d.heads, d.ffn, d.max_pos, d.ln_eps, d.pooling, d.flags | 1)
    lines, lines_small = nat.encoder_plan_describe(d, batch, seq), nat.encoder_plan_describe(small, batch, seq)
    new = [ln for ln in lines_small.splitlines() if ln.startswith("rope_qk_kernel") or re.match(r"gemm_(f16|panel)_kernel<4\b", ln)]
    assert len(new) == 2, lines_small                            # the two steps this family adds
    assert " lds=0" in new[0]                                    # the rotation: no LDS at all
    if cfg.hidden % 128 == 0:                                    # a width the panel kernel stages: its small-LDS form, <= 48 KB
        assert new[1].startswith("gemm_panel_kernel<4, ") and 0 < int(re.search(r"lds=(\d+)", new[1]).group(1)) <= 48 * 1024
    else:   # hidden 64 has no panel chunk: FFN-up falls to the tiled kernel, 64 KB of STATIC LDS (its line prints the dynamic 0) -- as
        # modes 0 / 1 of a BERT model of this width do; the flag's 48 KB does not hold for that fallback (include/crs_encoder.h)
        assert new[1].startswith("gemm_f16_kernel<4> ")
    if lines == lines_small:                                     # the same launches: the same bits
        ids, mask = golden[key + ".ids"], golden[key + ".mask"].astype(np.int32)
        b, hb = enc.forward(ids, mask.sum(1).astype(np.int32), return_hidden=True)
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(ha, hb)


# ---- the engine, with prefixes -------------------------------------------------------------------------------------------------
def test_engine_query_forward_rotates_and_carries_the_prefix(cuda):
    """retrieve_batch through the engine (graph-captured query forwards, CRS_ENC_SMALL_LDS) finds what search_batch finds for
    embeddings of a direct forward call on the PREFIXED questions -- and a forward with the identity rotation does not."""
    import torch
    from rag import RAGPipeline
    from rag.chunking import Chunk
    from rag.tokenizer import pad_batch

    class Stub:
        def generate(self, prompt, **kw):
            return "n/a"

    words = ("retrieval augmented generation language model quantization weights perplexity attention embedding cosine similarity "
             "vector index chunk context answer question compression memory latency throughput kernel softmax rotary gate").split()
    p = RAGPipeline({"embedding": {"model_name": "synthetic:tiny-nomic", "device": "cuda", "batch_size": 256, "normalize": True,
                                   "query_prefix": "search_query: ", "document_prefix": "search_document: "},
                     "retrieval": {"top_k": 5, "similarity_threshold": -1.0, "rerank": False, "diversity_penalty": 0.0, "batch_queries": 64},
                     "vector_store": {"collection_name": "nomic-e2e"}})
    p.setup(Stub())
    model = p.embedding_model
    assert model.shape.rotary_theta == 1000.0 and model.shape.gated and model.model.rope_table is not None and model.model.desc.flags == 6
    rng = np.random.default_rng(31)
    chunks = [Chunk(text=" ".join(rng.choice(words, size=int(rng.integers(4, 11)))) + f" {r}", chunk_id=f"c_{r}", start_char=0, end_char=1,
                    page_number=None) for r in range(2048)]
    emb_docs = model.embed_chunks_device(chunks)
    # the chunk methods embed "search_document: <text>", not the bare text (another batch composition: equal within the encoder's
    # cosine bound, not bit for bit)
    with_prefix = model.embed_device(["search_document: " + c.text for c in chunks[:8]])
    bare = model.embed_device([c.text for c in chunks[:8]])
    assert ((emb_docs[:8] * with_prefix).sum(1) > 1.0 - 2e-4).all().item() and ((emb_docs[:8] * bare).sum(1) < 1.0 - 1e-3).all().item()
    p.vector_store.create_index(chunks, emb_docs)
    questions = [" ".join(rng.choice(words, size=int(rng.integers(3, 8)))) + f" {q}" for q in range(128)]
    got = p.retrieve_batch(questions)
    assert p.retriever._engine is not None, "the call did not take the engine"
    toks = model.tokenize(questions, kind="query")
    assert toks == model.tokenize(["search_query: " + q for q in questions]) and toks != model.tokenize(questions)
    assert max(len(t) for t in toks) <= 16
    ids, lens = pad_batch(toks, model.tokenizer.pad_id, short_steps=(16,))
    assert ids.shape == (128, 16)
    emb = model.model.forward(ids, lens)
    want = p.vector_store.search_batch(emb, top_k=5)["ids"]
    assert [[c["chunk_id"] for c in g] for g in got] == want
    # the same weights with the identity rotation (cos 1, sin 0): other embeddings, other lists
    keep = model.model.rope_table
    ident = torch.zeros_like(keep)
    ident[:, : keep.shape[1] // 2] = 1.0
    model.model.rope_table = ident
    plain = p.vector_store.search_batch(model.model.forward(ids, lens), top_k=5)["ids"]
    model.model.rope_table = keep
    assert sum(a != b for a, b in zip(plain, want)) > 32


def test_device_tokenisation_with_a_prefix_gives_the_host_ids(cuda, tmp_path):
    import torch
    from rag.embedding import EmbeddingModel
    d = str(tmp_path / "nomic")
    nc.write_nomic_dir(d, "hub")
    cfgs = {"model_name": d, "batch_size": 32, "query_prefix": "query: ", "document_prefix": "context text: "}
    host, device = EmbeddingModel({**cfgs, "tokenize": "host"}), EmbeddingModel({**cfgs, "tokenize": "device"})
    assert host.shape.gated and host.shape.rotary_theta == 1000.0 and host.shape.max_seq == 48
    texts = ["The quick brown fox jumps over the lazy dog.", "  retrieval augmented generation ", "", "zzzz qqq!", "the " * 60] * 8
    for kind in (None, "query", "document"):
        want = host.tokenize(texts, kind=kind)
        ids, lens = device.tokenize_device(texts, kind=kind)
        ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
        assert lens.tolist() == [len(t) for t in want]
        for row, n, t in zip(ids, lens, want):
            assert row[:n].tolist() == t and (row[n:] == host.tokenizer.pad_id).all()
        assert torch.equal(host.embed_device(texts, kind=kind), device.embed_device(texts, kind=kind))
    assert not torch.equal(host.embed_device(texts[:4], kind="query"), host.embed_device(texts[:4]))
