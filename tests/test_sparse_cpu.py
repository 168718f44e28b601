"""CPU: learned sparse retrieval without a device.  The loader's name mapping (tied decoder, both spellings of the bias) and its
error for a directory without the MLM head; tests/_sparse_ref.py's head against what `transformers` computed
(tests/golden/splade.npz, tools/make_splade_golden.py); the compaction reference's properties; the synthetic models' bias shift
on the fp64 reference; launch cutting and sparse_rows over a CPU collection with the natives replaced by the references; the
retriever's `sparse_model` key; the launch plan's geometry; the new entry points declared, exported, bound, and refusing bad
arguments before any HIP call."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _sparse_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "splade.npz")
U = ref.U32


def _golden():
    z = np.load(GOLDEN)
    state = {k[3:]: z[k] for k in z.files if k.startswith("w::")}
    cfg = json.loads(bytes(z["config"]).decode())
    return z, state, cfg


# ---- the loader ------------------------------------------------------------------------------------------------------------------------
def _write_mlm_dir(path, state, cfg):
    """A BertForMaskedLM directory: _modeldir's tokenizer files and vocabulary, the golden's config and the given state dict."""
    from safetensors.numpy import save_file
    from _modeldir import write_model_dir
    write_model_dir(str(path))
    json.dump(cfg, open(os.path.join(path, "config.json"), "w"))
    save_file({k: np.ascontiguousarray(v) for k, v in state.items()}, os.path.join(path, "model.safetensors"))


def test_loader_maps_the_checkpoint_names(tmp_path):
    from rag import sparse as sp
    z, state, cfg = _golden()
    emb = state["bert.embeddings.word_embeddings.weight"]
    variants = {
        "tied": dict(state),                                                                  # no decoder.weight: tied
        "untied": dict(state, **{"cls.predictions.decoder.weight": emb * 2.0}),
        "decoder_bias": {("cls.predictions.decoder.bias" if k == "cls.predictions.bias" else k): v for k, v in state.items()},
        "both_biases": dict(state, **{"cls.predictions.decoder.bias": state["cls.predictions.bias"]}),
    }
    for name, st in variants.items():
        d = tmp_path / name
        _write_mlm_dir(d, st, cfg)
        shape, w, tok, _ = sp.load_sparse_dir(str(d))
        assert (shape.vocab_size, shape.hidden, shape.layers, shape.heads, shape.ffn, shape.max_pos) == (len(emb), 64, 2, 4, 128, 64), name
        assert not any(k.startswith("bert.") for k in w) and sp.DEC_B_ALT not in w, name
        assert np.array_equal(w[sp.WORD_EMB], emb), name
        assert np.array_equal(w[sp.DEC_W], emb * 2.0 if name == "untied" else emb), name
        assert np.array_equal(w[sp.DEC_B], state["cls.predictions.bias"]), name
        for short, full in ((sp.T_DENSE_W, "cls.predictions.transform.dense.weight"), (sp.T_LN_B, "cls.predictions.transform.LayerNorm.bias")):
            assert np.array_equal(w[short], state[full]), name
        assert tok.encode("the fox", 16)[0] == 2                                               # [CLS] of the directory's vocabulary
        enc = sp.SparseEncoder({"model_path": str(d), "max_seq": 32})
        assert enc.vocab_size == len(emb) and enc.skip_ids == [0, 2, 3] and enc.max_seq == 32    # [PAD] [CLS] [SEP]


def test_a_directory_without_the_head_is_refused_by_name(tmp_path):
    from rag import sparse as sp
    from _modeldir import write_model_dir
    write_model_dir(str(tmp_path / "plain"))                                                   # a sentence encoder: bert.* alone
    with pytest.raises(NotImplementedError) as e:
        sp.SparseEncoder(str(tmp_path / "plain"))
    for name in (sp.T_DENSE_W, sp.T_LN_W, sp.DEC_B):
        assert name in str(e.value)
    assert sp.DEC_W not in str(e.value)                                                        # tied: not missing
    z, state, cfg = _golden()
    distil = {k.replace("cls.predictions.transform.dense", "vocab_transform").replace("cls.predictions.transform.LayerNorm", "vocab_layer_norm")
              .replace("cls.predictions.bias", "vocab_projector.bias"): v for k, v in state.items()}
    _write_mlm_dir(tmp_path / "distil", distil, cfg)
    with pytest.raises(NotImplementedError, match="cls.predictions.transform.dense.weight"):
        sp.load_sparse_dir(str(tmp_path / "distil"))
    with pytest.raises(FileNotFoundError, match="synthetic:tiny-splade"):
        sp.SparseEncoder("naver/splade-v3")
    with pytest.raises(ValueError, match="tokenize"):
        sp.SparseEncoder({"model_name": "synthetic:tiny-splade", "tokenize": "gpu"})


# ---- the head reference against transformers --------------------------------------------------------------------------------------------
def test_head_reference_agrees_with_transformers():
    """Both sides are exact arithmetic on the same fp32 inputs up to summation order and rounding, so the bounds are derived from
    K 2^-24 sum|a w| and nothing is tuned.  Stage 1, the transform from the golden hidden states: the K = 64 projection of
    `transformers` (fp32) is off by at most (K + 1) u S, S = sum_k |w_jk h_k| + |b_j|; GELU has slope <= 1.13 and torch's erf is
    good to 4 u: e_x = 1.13 (K + 1) u S + 4 u |x|; LayerNorm subtracts a mean carrying at most the largest e_x and scales by
    |gamma| / std, and its own fp32 steps add 8 u (|y| + |beta|).  Stage 2, the pool from the golden transform outputs: (K + 1) u
    (sum|t w| + |bias|) on a logit, carried through max and log1p (1-Lipschitz), plus 2 ulp for torch's fp32 log1p and the store."""
    z, st, cfg = _golden()
    K = 64
    hidden, lens = z["hidden"], z["lens"]
    w_t, b_t = st["cls.predictions.transform.dense.weight"], st["cls.predictions.transform.dense.bias"]
    g, be = st["cls.predictions.transform.LayerNorm.weight"], st["cls.predictions.transform.LayerNorm.bias"]
    w_d, bias = st["bert.embeddings.word_embeddings.weight"], st["cls.predictions.bias"]
    worst = [0.0, 0.0]
    tol_t = np.zeros(hidden.shape, dtype=np.float64)
    for b in range(hidden.shape[0]):
        n = int(lens[b])
        h = hidden[b, :n].astype(np.float64)
        want = ref.transform_ref(h, w_t, b_t, g, be, cfg["layer_norm_eps"])
        S = np.abs(h) @ np.abs(w_t.astype(np.float64)).T + np.abs(b_t)
        x = h @ w_t.astype(np.float64).T + b_t
        gx = 0.5 * x * (1.0 + ref._erf(x / np.sqrt(2.0)))
        e_x = 1.13 * (K + 1) * U * S + 4 * U * np.abs(gx)
        std = gx.std(-1, keepdims=True)
        tol = 2.0 * e_x.max(-1, keepdims=True) * np.abs(g) / std + 8 * U * (np.abs(want) + np.abs(be))
        err = np.abs(z["transform"][b, :n].astype(np.float64) - want)
        worst[0] = max(worst[0], float((err / tol).max()))
        assert (err <= tol).all(), (b, float((err / tol).max()))
        tol_t[b, :n] = tol
    got, absdot = ref.pool_ref(z["transform"].astype(np.float64), lens, w_d, bias)
    tol = (K + 1) * U * (absdot + np.abs(bias)) + 2 * np.spacing(np.abs(got).astype(np.float32)).astype(np.float64)
    err = np.abs(z["weights"].astype(np.float64) - got)
    worst[1] = float((err / tol).max())
    assert (err <= tol).all(), worst
    assert (((z["weights"] > 0) == (got > 0)) | (got <= tol)).all()                            # the same support, up to a weight within the bound of 0
    print(f"transformers vs fp64 reference: worst error / bound, transform {worst[0]:.3f}, weights {worst[1]:.3f}; "
          f"positive ids per text {(got > 0).sum(1).tolist()}")
    assert (got > 0).sum() > 50
    # chained from the hidden states, nothing rounded in between: within what stage 1's tolerance can move a logit
    whole = ref.head_ref(hidden, lens, w_t, b_t, g, be, cfg["layer_norm_eps"], w_d, bias)
    moved = np.stack([(tol_t[b, :max(int(lens[b]), 1)] @ np.abs(w_d.astype(np.float64)).T).max(0) for b in range(hidden.shape[0])])
    assert (np.abs(whole - got) <= moved).all()


# ---- compaction --------------------------------------------------------------------------------------------------------------------------
def test_compaction_reference_properties():
    rng = np.random.default_rng(0)
    row = np.zeros(500, dtype=np.float32)
    at = 10 + rng.choice(490, size=120, replace=False)
    row[at] = rng.random(120).astype(np.float32) + 0.01
    row[at[:30]] = 0.5                                                                         # thirty-way tie
    row[7], row[8], row[9] = -1.0, np.nan, -0.0
    for cap in (1, 64, 119, 120, 121, 1024):
        ids, w, n = ref.compact_ref(row, cap)
        assert n == min(cap, 120) and (ids[n:] == -1).all() and (w[n:] == 0).all()
        assert (np.diff(ids[:n]) > 0).all() and (w[:n] == row[ids[:n]]).all() and (w[:n] > 0).all()
        kept, dropped = set(ids[:n].tolist()), set(at.tolist()) - set(ids[:n].tolist())
        if dropped:
            lo = min(row[i] for i in kept)
            assert all(row[i] <= lo for i in dropped)
            assert all(i > max(j for j in kept if row[j] == lo) for i in dropped if row[i] == lo)     # ties: the lower ids stay
    ids, w, n = ref.compact_ref(row, 64, skip_ids=(int(at[0]), int(at[31])))
    assert int(at[0]) not in ids and int(at[31]) not in ids and n == 64
    assert ref.compact_ref(np.zeros(10, dtype=np.float32), 4)[2] == 0


# ---- the synthetic models --------------------------------------------------------------------------------------------------------------
def test_synthetic_bias_shift_gives_a_few_to_a_few_dozen_terms_with_margin():
    """On the fp64 reference of synthetic:tiny-splade over the shared corpus: every non-empty text activates 1 .. 64 ids and the
    median lies in 3 .. 40; and the reference alone has the margin the GPU test relies on: the (text, id) pairs whose weight lies
    within the device's rounding bound of 0 (they could appear on one side only) are fewer than 1 % of the positive ones, for the
    projection's bound (pool_bound) and for the end-to-end bound of model_reference alike.  (No
    text reaches the cap of 256, so no id sits near a cap-th weight.)"""
    from rag.sparse import SparseEncoder
    enc = SparseEncoder("synthetic:tiny-splade")
    texts = ref.corpus(300)                                                                    # the GPU test's corpus
    ids = enc.tokenize(texts)
    w, absdot, e2e = ref.model_reference(enc._weights, enc.shape, ids, with_bound=True)
    w[:, enc.skip_ids] = 0.0
    n_pos = (w > 0).sum(1)
    print(f"tiny-splade, fp64 reference: positive ids per text min {n_pos.min()} median {int(np.median(n_pos))} max {n_pos.max()}")
    assert n_pos.max() <= 64 and 3 <= np.median(n_pos) <= 40 and (n_pos[[i for i, t in enumerate(ids) if len(t) > 6]] >= 1).all()
    near_zero = (w > 0) & (w <= ref.pool_bound(absdot, w, enc.shape.hidden))
    assert near_zero.sum() <= 0.01 * (w > 0).sum()
    near_zero = (w > 0) & (w <= e2e[:, None])                                                  # the end-to-end bound of model_reference
    print(f"end-to-end bound: median {np.median(e2e):.2e} max {e2e.max():.2e}; {near_zero.sum()} of {(w > 0).sum()} positive weights within it of 0")
    assert near_zero.sum() <= 0.01 * (w > 0).sum() and 0 < e2e.max() < 1e-2
    from rag import sparse as sp
    assert sp._KNOWN_SPARSE["splade-base"]["vocab_size"] == 30522 and sp._KNOWN_SPARSE["splade-base"]["hidden"] == 768


# ---- the store: launch cutting, the index's life cycle ------------------------------------------------------------------------------------
class _FakeEncoder:
    """A SparseEncoder stand-in on CPU tensors: a text's terms are the crc32 of its words into 500 ids, weight 1 + (count of the word)."""
    vocab_size = 500

    def __init__(self):
        self.calls = []

    def encode_device(self, texts, max_terms):
        import torch
        import zlib
        self.calls.append(len(texts))
        n = len(texts)
        ids = torch.full((n, max_terms), -1, dtype=torch.int32)
        w = torch.zeros((n, max_terms), dtype=torch.float32)
        counts = torch.zeros(n, dtype=torch.int32)
        for i, t in enumerate(texts):
            row = np.zeros(self.vocab_size, dtype=np.float32)
            for word in str(t).lower().split():
                row[zlib.crc32(word.encode()) % self.vocab_size] += 1.0
            row[row > 0] += 1.0
            a, b, c = ref.compact_ref(row, max_terms)
            ids[i], w[i], counts[i] = torch.from_numpy(a), torch.from_numpy(b), c
        return ids, w, counts

    encode_docs_device = encode_queries_device = encode_device


def _store(docs, cfg=None):
    from rag.indexing import SlabCollection, VectorStore
    store = VectorStore(dict({"collection_name": "sparse", "max_index_bytes": 1 << 30}, **(cfg or {})))
    col = SlabCollection("sparse", "fp16", False, ["cpu"])
    col.ids.extend(f"c{i}" for i in range(len(docs)))
    col.documents.extend(docs)
    col.metadatas.extend({} for _ in docs)
    store.collection = store._adopt(col)
    return store


def _patch(monkeypatch):
    import torch
    from rag import _native as nat
    launches = []

    def sparse_topk(doc_off, doc_tok, doc_w, n_rows, q_off, q_tok, q_w, k, workspace=None, out_scores=None, out_rows=None):
        assert doc_off.dtype == torch.int64 and doc_tok.dtype == torch.int32 and doc_w.dtype == torch.float32 and q_off.dtype == torch.int64
        launches.append((q_off.shape[0] - 1, int(q_tok.shape[0])))
        qo, qt, qw = q_off.numpy(), q_tok.numpy(), q_w.numpy()
        rows = [(qt[qo[i]:qo[i + 1]], qw[qo[i]:qo[i + 1]]) for i in range(len(qo) - 1)]
        rows = [(t[t >= 0], w[t >= 0]) for t, w in rows]                                      # the padded slots match no row
        s, r = ref.sparse_topk_ref(doc_off.numpy(), doc_tok.numpy(), doc_w.numpy(), n_rows, *ref.csr_of(rows), k)
        out_scores.copy_(torch.from_numpy(s))
        out_rows.copy_(torch.from_numpy(r))
        return out_scores, out_rows

    monkeypatch.setattr(nat, "sparse_topk", sparse_topk)
    return launches


def _want(enc, docs, queries, k, doc_terms=256, query_terms=64):
    d = enc.encode_device(docs, doc_terms)
    q = enc.encode_device(queries, query_terms)
    rows = lambda e: [(i[i >= 0].numpy(), w[i >= 0].numpy()) for i, w in zip(e[0], e[1])]      # noqa: E731
    off, tok, w = ref.csr_of(rows(d))
    return ref.sparse_topk_ref(off, tok, w, len(docs), *ref.csr_of(rows(q)), k)


def test_sparse_rows_cuts_a_batch_at_64_queries_and_at_the_pair_cap(monkeypatch):
    from rag import _native as nat
    docs, queries = ref.corpus(150), ref.queries(130)
    store = _store(docs)
    launches = _patch(monkeypatch)
    enc = _FakeEncoder()
    store.attach_sparse_encoder(enc)
    scores, rows = store.sparse_rows(queries, 10)
    assert launches == [(64, 4096), (64, 4096), (2, 128)] and store.last_sparse == {"queries": 130, "query_terms": 64, "launches": 3}
    want_s, want_r = _want(_FakeEncoder(), docs, queries, 10)
    assert (rows == want_r).all() and (scores.view(np.int32) == want_s.view(np.int32)).all()
    assert (rows[:, 0] >= 0).all()
    # more terms a query: fewer queries a launch, never above the pair cap
    wide = _store(docs, {"sparse_query_terms": 1024})
    wide.attach_sparse_encoder(_FakeEncoder())
    del launches[:]
    wide.sparse_rows(queries[:9], 5)
    assert launches == [(4, 4096), (4, 4096), (1, 1024)] and all(p <= nat.BM25_MAX_PAIRS for _, p in launches)
    got = store.search_sparse_batch(queries[:3], top_k=4)
    assert set(got) == {"ids", "documents", "metadatas", "scores"} and got["ids"][0] == [f"c{r}" for r in want_r[0, :4]]
    assert got["scores"][0] == want_s[0, :4].astype(np.float64).tolist()
    for bad in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match="top_k"):
            store.sparse_rows(["x"], bad)
    s0, r0 = store.sparse_rows([], 5)
    assert s0.shape == r0.shape == (0, 5)
    with pytest.raises(ValueError, match="sparse_query_terms"):
        _store(docs, {"sparse_query_terms": 1025})


def test_index_is_extended_by_appends_dropped_by_changes_and_guarded(monkeypatch):
    docs = ref.corpus(80)
    store = _store(docs[:50])
    _patch(monkeypatch)
    enc = _FakeEncoder()
    with pytest.raises(ValueError, match="attach_sparse_encoder"):
        store.sparse_index()
    index = store.sparse_index(enc)
    assert enc.calls == [50] and index.n_rows == 50 and index.offsets_dev.dtype.is_floating_point is False
    assert index.tokens.dtype.itemsize == 4 and index.n_terms == int(index.offsets[-1]) and (np.diff(index.offsets) >= 0).all()
    col = store.collection
    col.ids.extend(f"c{i}" for i in range(50, 80)); col.documents.extend(docs[50:]); col.metadatas.extend({} for _ in docs[50:])
    again = store.sparse_index()
    assert again is index and enc.calls == [50, 30] and index.n_rows == 80                     # the old rows are not encoded again
    want = _want(_FakeEncoder(), docs, ref.queries(5), 8)
    got = store.sparse_rows(ref.queries(5), 8)
    assert (got[1] == want[1]).all() and (got[0].view(np.int32) == want[0].view(np.int32)).all()
    col.documents[3] = "an entirely new text about kernels"
    col._drop_derived(ids_changed=False, documents_changed=True)
    assert "_sp" not in col.__dict__
    fresh = store.sparse_index()
    assert fresh is not index and fresh.n_rows == 80
    col._drop_derived(ids_changed=False, metadata_changed=True, documents_changed=False)
    assert store.sparse_index() is fresh                                                       # a metadata change keeps it
    # the guard: rows x sparse_doc_terms x 8 bytes, before any encoding
    small = _store(docs, {"max_index_bytes": 80 * 256 * 8 - 1})
    counted = _FakeEncoder()
    with pytest.raises(ValueError, match="max_index_bytes"):
        small.sparse_index(counted)
    assert counted.calls == []
    sharded = _store(docs)
    sharded.sharded = True
    with pytest.raises(NotImplementedError, match="one device"):
        sharded.sparse_index(_FakeEncoder())


# ---- the retriever -------------------------------------------------------------------------------------------------------------------
class _NoStore:
    collection = None


def test_sparse_model_without_hybrid_raises():
    from rag.retrieval import ContextRetriever
    for cfg in ({"sparse_model": "synthetic:tiny-splade"}, {"sparse_model": {"model_name": "synthetic:tiny-splade"}, "hybrid": False}):
        with pytest.raises(ValueError, match="hybrid"):
            ContextRetriever(_NoStore(), None, cfg)
    with pytest.raises(ValueError, match="sparse_rows"):
        ContextRetriever(_NoStore(), None, {"sparse_model": "synthetic:tiny-splade", "hybrid": True})
    plain = ContextRetriever(_NoStore(), None, {"hybrid": True})
    assert plain.sparse_encoder is None and plain.last_sparse == {"queries": 0, "query_terms": 0, "launches": 0}
    assert plain.last_hybrid == {"lists": 0, "lexical_only_hits": 0}                           # gains nothing


# ---- the launch plan --------------------------------------------------------------------------------------------------------------------
def test_launch_plan_covers_the_shapes_exactly():
    from rag import _native as nat
    shapes = [(b, s, 64, v) for b in (1, 5, 9) for s in (1, 17, 48) for v in (1, 10, 16, 250, 127, 128, 129, 266)]
    shapes += [(2, 32, 768, 30522), (64, 256, 768, 30522), (64, 32, 768, 30522), (1, 1, 1024, 1 << 20), (8192, 512, 384, 250037)]
    for batch, seq, hidden, vocab in shapes:
        p = nat.mlm_pool_plan(batch, seq, hidden, vocab)
        tokens = batch * seq
        assert p["tokens"] == tokens and p["tile_n"] == ref.TILE_N
        assert (p["grid_m"] - 1) * p["tile_m"] < tokens <= p["grid_m"] * p["tile_m"] == p["tokens_padded"]
        assert (p["grid_n"] - 1) * p["tile_n"] < vocab <= p["grid_n"] * p["tile_n"]
        assert p["pool_grid"] == p["grid_m"] * p["grid_n"] < 2 ** 31 and p["pool_threads"] == 256
        assert p["pool_lds_bytes"] <= 160 * 1024 and p["xform_lds_bytes"] <= 160 * 1024
        assert p["xform_grid"] * 32 == p["tokens_padded"] and hidden % p["tile_k"] == 0
        assert (p["ew_grid_x"] - 1) * p["ew_threads"] < vocab <= p["ew_grid_x"] * p["ew_threads"]
        assert p["t16_bytes"] == p["tokens_padded"] * hidden * 2 <= p["workspace_bytes"] == nat.mlm_workspace_bytes(batch, seq, hidden, vocab)
        assert p["workspace_bytes"] % 256 == 0
    for bad in ((0, 8, 64, 10), (1, 0, 64, 10), (1, 8, 96, 10), (1, 8, 64, 0), (1, 8, 64, (1 << 20) + 1), (1 << 12, 1 << 11, 64, 10)):
        with pytest.raises(nat.NativeError):
            nat.mlm_pool_plan(*bad)


# ---- boundary --------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    import torch
    from rag import _native as nat
    import rag._encoder  # noqa: F401
    strip = lambda p: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", p)).read(), flags=re.S)      # noqa: E731
    hip, encoder = strip("crs_hip.h"), strip("crs_encoder.h")
    lib = nat.load()
    for name, header in (("crs_sparse_compact", hip), ("crs_sparse_topk", hip), ("crs_sparse_workspace_bytes", hip),
                         ("crs_mlm_sparse_pool", encoder), ("crs_mlm_workspace_bytes", encoder), ("crs_mlm_pool_plan", encoder)):
        assert re.search(r"\bint %s\s*\(" % name, header), f"{name} not declared"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in nat.exported_symbols()
    assert lib.crs_abi_version() == 3
    assert re.search(r"#define CRS_SPARSE_MAX_TERMS (\d+)", hip).group(1) == str(nat.SPARSE_MAX_TERMS) == "1024"
    assert re.search(r"#define CRS_SPARSE_MAX_SKIP (\d+)", hip).group(1) == str(nat.SPARSE_MAX_SKIP)
    assert nat.has_sparse() and callable(nat.mlm_sparse_pool) and callable(nat.sparse_compact) and callable(nat.sparse_topk)
    assert str(torch.ops.crs.sparse_topk.default._schema) == \
        ("crs::sparse_topk(Tensor doc_offsets, Tensor doc_tokens, Tensor doc_weights, int n_rows, Tensor q_offsets, Tensor q_tokens, "
         "Tensor q_weights, int k, Tensor(a!) workspace, Tensor(b!) out_scores, Tensor(c!) out_rows) -> ()")
    makefile = open(os.path.join(ROOT, "compressed-rag-suite_amd", "csrc", "Makefile")).read()
    assert all(f in makefile for f in ("mlm_pool.hip", "sparse_compact.hip", "sparse_scan.hip", "mlm_plan.o"))
    fields = re.search(r"typedef struct crs_mlm_plan \{(.*?)\} crs_mlm_plan;", encoder, flags=re.S).group(1)
    declared = [n.strip() for line in fields.split(";") if line.strip() for n in line.split(None, 1)[1].split(",")]
    assert declared == [n for n, _ in nat.MlmPlan._fields_]                                    # the ctypes mirror, field for field


@pytest.mark.parametrize("source,kernels", [("mlm_pool.hip", 10), ("sparse_compact.hip", 2), ("sparse_scan.hip", 2)])
def test_kernels_use_no_scratch(source, kernels):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_resources.py"), source], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "0 violation(s)" in r.stdout and f"{kernels} kernels in 1 files" in r.stdout, r.stdout


def test_argument_validation_without_gpu():
    from rag import _native as nat
    lib = nat.load()
    buf = (ctypes.c_char * 8192)()                     # host memory standing in for device pointers: never dereferenced
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)
    EINVAL, ENOSPC = -1, -2

    class Head(ctypes.Structure):
        _fields_ = [("hidden", ctypes.c_int32), ("vocab", ctypes.c_int32), ("max_pos", ctypes.c_int32), ("ln_eps", ctypes.c_float)] + \
                   [(n, ctypes.c_void_p) for n in ("transform_w16", "transform_bias", "ln_gamma", "ln_beta", "decoder_w16", "decoder_bias")]

    def pool(batch=2, seq=8, hidden_dev=p, lens=p, ws=p, ws_bytes=1 << 20, out=p, vp=100, head=True, **fields):
        h = Head(64, 100, 512, 1e-12, p, p, p, p, p, p)
        for k, v in fields.items():
            setattr(h, k, v)
        return lib.crs_mlm_sparse_pool(hidden_dev, lens, batch, seq, ctypes.byref(h) if head else None, ws, ws_bytes, out, vp, None)

    for bad, word in (({"batch": 0}, b"batch"), ({"seq": 0}, b"seq"), ({"seq": 513}, b"max_pos"), ({"vocab": 0}, b"vocab"),
                      ({"hidden": 96}, b"hidden"), ({"vp": 99}, b"vp"), ({"hidden_dev": None}, b"null pointer"), ({"lens": None}, b"null pointer"),
                      ({"out": None}, b"null pointer"), ({"head": False}, b"null head"), ({"transform_w16": None}, b"null pointer"),
                      ({"decoder_bias": None}, b"null pointer"), ({"ln_gamma": None}, b"null pointer"), ({"ws": None}, b"workspace"),
                      ({"ws": ctypes.c_void_p(p.value + 16)}, b"workspace"), ({"hidden_dev": ctypes.c_void_p(p.value + 4)}, b"16-byte")):
        assert pool(**bad) == EINVAL, bad
        assert word in lib.crs_last_error(), (bad, lib.crs_last_error())
    assert pool(ws_bytes=nat.mlm_workspace_bytes(2, 8, 64, 100) - 1) == ENOSPC

    c_names = ("weights", "batch", "vocab", "vp", "cap", "skip", "n_skip", "ids", "out_w", "counts")
    c_good = dict(weights=p, batch=2, vocab=100, vp=100, cap=64, skip=p, n_skip=3, ids=p, out_w=p, counts=p)
    for bad, word in (({"batch": 0}, b"batch"), ({"vocab": 0}, b"vocab"), ({"vp": 99}, b"vp"), ({"cap": 0}, b"cap"), ({"cap": 1025}, b"CRS_SPARSE_MAX_TERMS"),
                      ({"n_skip": -1}, b"n_skip"), ({"n_skip": 17}, b"n_skip"), ({"weights": None}, b"null pointer"), ({"skip": None}, b"null pointer"),
                      ({"ids": None}, b"null pointer"), ({"out_w": None}, b"null pointer"), ({"counts": None}, b"null pointer")):
        args = dict(c_good, **bad)
        assert lib.crs_sparse_compact(*[args[n] for n in c_names], None) == EINVAL, bad
        assert word in lib.crs_last_error(), (bad, lib.crs_last_error())

    need = nat.sparse_workspace_bytes(4, 10, 1000)
    assert need == nat.bm25_workspace_bytes(4, 10, 1000)
    t_names = ("doc_off", "doc_tok", "doc_w", "n_rows", "n_doc_tok", "q_off", "q_tok", "q_w", "nq", "n_q_tok", "k", "ws", "ws_bytes", "out_s", "out_r")
    t_good = dict(doc_off=p, doc_tok=p, doc_w=p, n_rows=1000, n_doc_tok=9000, q_off=p, q_tok=p, q_w=p, nq=4, n_q_tok=12, k=10, ws=p, ws_bytes=need,
                  out_s=p, out_r=p)
    for bad, word in (({"nq": 0}, b"nq"), ({"nq": 65}, b"nq"), ({"k": 0}, b"k"), ({"k": 65}, b"k"), ({"n_rows": -1}, b"n_rows"),
                      ({"n_rows": 2 ** 31}, b"n_rows"), ({"n_doc_tok": -1}, b"n_doc_tokens"), ({"n_q_tok": 4097}, b"CRS_BM25_MAX_PAIRS"),
                      ({"doc_off": None}, b"null pointer"), ({"doc_tok": None}, b"null pointer"), ({"doc_w": None}, b"null pointer"),
                      ({"q_off": None}, b"null pointer"), ({"q_w": None}, b"null pointer"), ({"out_s": None}, b"null pointer"),
                      ({"ws": None}, b"workspace"), ({"ws": ctypes.c_void_p(p.value + 8)}, b"workspace")):
        args = dict(t_good, **bad)
        assert lib.crs_sparse_topk(*[args[n] for n in t_names], None) == EINVAL, bad
        assert word in lib.crs_last_error(), (bad, lib.crs_last_error())
    args = dict(t_good, ws_bytes=need - 1)
    assert lib.crs_sparse_topk(*[args[n] for n in t_names], None) == ENOSPC
