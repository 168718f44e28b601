"""GPU: crs_unigram_encode (csrc/unigram.hip) against the pure-Python restatement rag.tokenizer.UnigramTokenizer on the edge
corpus of tests/_unigram_cases.py, at every row width; two launches give the same bytes; EmbeddingModel with
rag.embedding.tokenize 'device' hands the encoder the blocks that 'host' does and returns the same bits."""
import numpy as np
import pytest

import _unigram_cases as uc
import _xlmr_cases as xc

pytestmark = pytest.mark.gpu

PATHS = {"nfkc": uc.NFKC_JSON, "spm": uc.SPM_JSON}
_SIDE = {}


def side(kind, cuda):
    """(restatement, device tokeniser) of a fixture, built once for the module."""
    if kind not in _SIDE:
        from rag import _unigram as ug
        tok = uc.restatement(PATHS[kind])
        _SIDE[kind] = (tok, ug.device_tokenizer(tok, cuda))
        assert isinstance(_SIDE[kind][1], ug.UnigramDeviceTokenizer)
    return _SIDE[kind]


def corpus():
    from rag import _native as nat
    return uc.edge_corpus(nat.UNIGRAM_MAX_WORD, nat.UNIGRAM_TILE_BYTES)


def run(dt, texts, width):
    import torch
    ids, lens, flags, host = dt.encode(texts, width)
    torch.cuda.synchronize()
    assert host == []
    return ids.cpu().numpy(), lens.cpu().numpy(), flags.cpu().numpy()


def check_against_restatement(kind, cuda, width):
    from rag import _native as nat
    from rag import _unigram as ug
    tok, dt = side(kind, cuda)
    names, texts = [n for n, _ in corpus()], [t for _, t in corpus()]
    ids, lens, flags = run(dt, texts, width)
    assert ids.shape == (len(texts), width) and ids.dtype == np.int32
    for r, (name, text) in enumerate(zip(names, texts)):
        emu = ug.emulate_encode(text, dt.table, dt.vocab, dt.spec, width)
        if flags[r]:
            assert emu is None, (kind, width, name)
            continue
        # a text the emulation flags may pass unflagged only when the row filled up before the kernel read that far
        assert emu is not None or (lens[r] == width and len(text.encode()) > 8), (kind, width, name)
        want = tok.encode(text, width)
        assert lens[r] == len(want), (kind, width, name)
        assert ids[r, : lens[r]].tolist() == want, (kind, width, name)
        assert (ids[r, lens[r]:] == tok.pad_id).all(), (kind, width, name)
    if width == 64:          # every flagged text of the corpus is flagged within its first 62 ids, or is shorter than that
        assert {n for n, f in zip(names, flags) if f} == uc.FLAGGED
        assert flags[names.index("word-cap+1")] == 1 and flags[names.index("word-cap")] == 0
    assert nat.UNIGRAM_TILE_BYTES == 1024 and nat.UNIGRAM_MAX_WORD == 128


@pytest.mark.parametrize("width", uc.WIDTHS)
def test_op_equals_the_restatement_nfkc(cuda, width):
    check_against_restatement("nfkc", cuda, width)


@pytest.mark.parametrize("width", uc.WIDTHS)
def test_op_equals_the_restatement_precompiled(cuda, width):
    pytest.importorskip("tokenizers")
    check_against_restatement("spm", cuda, width)


def test_op_equals_the_golden_ids(cuda):
    """The same rows against the ids the `tokenizers` library wrote into tests/golden/unigram_ids.json.xz."""
    g = uc.load_json(uc.IDS_JSON)
    assert g["texts"] == [t for _, t in corpus()]
    _, dt = side("nfkc", cuda)
    for width in uc.WIDTHS:
        ids, lens, flags = run(dt, g["texts"], width)
        for r, want in enumerate(g["ids"][f"nfkc.{width}"]):
            if not flags[r]:
                assert ids[r, : lens[r]].tolist() == want, (width, g["names"][r])


def test_two_launches_give_identical_bytes(cuda):
    _, dt = side("nfkc", cuda)
    texts = [t for _, t in corpus()]
    a, b = run(dt, texts, 64), run(dt, texts, 64)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_random_texts_and_a_wide_row(cuda):
    """500 seeded texts in one launch, and one long text at a row wider than two tiles' worth of ids."""
    from rag import _unigram as ug
    tok, dt = side("nfkc", cuda)
    allowed = np.nonzero(~dt.table.fallback_mask())[0]
    texts = uc.random_texts(500, 21, allowed) + ["hello world the quick fox ab cd axyb " * 90]
    ids, lens, flags = run(dt, texts, 2048)
    assert not flags.any()
    for r, text in enumerate(texts):
        want = tok.encode(text, 2048)
        assert ids[r, : lens[r]].tolist() == want, ascii(text[:60])
    # the long text spans four tiles and its row holds all of its ids: nothing was cut
    assert len(texts[-1].encode()) > 3 * 1024 and lens[-1] == len(tok.encode(texts[-1], 1 << 20)) < 2048


def test_bad_arguments_are_einval(cuda):
    import torch
    from rag import _native as nat
    _, dt = side("nfkc", cuda)
    blob = torch.zeros(4, dtype=torch.uint8, device=cuda)
    off = torch.tensor([0, 4], dtype=torch.int64, device=cuda)
    sp = dt.spec
    args = lambda **kw: dict(dict(max_probe=dt.vocab.max_probe, lmax=dt.vocab.lmax, opts=dt.opts, max_len=8), **kw)      # noqa: E731
    for bad in (args(max_len=1), args(lmax=nat.UNIGRAM_MAX_WORD + 1), args(max_probe=0), args(opts=16)):
        with pytest.raises(nat.NativeError):
            nat.unigram_encode(blob, off, 4, dt.d_table, dt.d_rep, dt.d_slots, dt.d_scores, dt.d_pool, bad["max_probe"], bad["lmax"],
                               sp.unk_score, bad["opts"], sp.unk_id, sp.cls_id, sp.sep_id, sp.pad_id, bad["max_len"])


# ---- EmbeddingModel ------------------------------------------------------------------------------------------------------------------
def _embed_and_capture(model, texts):
    """(embeddings, [(ids, lens) of every HipEncoder.forward call])"""
    import torch
    calls = []
    real = model.model.forward

    def forward(ids, lens, *args, **kwargs):
        as_np = lambda x: x.detach().cpu().numpy().copy() if isinstance(x, torch.Tensor) else np.array(x)   # noqa: E731
        calls.append((as_np(ids).astype(np.int32), as_np(lens).astype(np.int32)))
        return real(ids, lens, *args, **kwargs)

    model.model.forward = forward
    try:
        emb = model.embed_device(texts)
        torch.cuda.synchronize()
        return emb.cpu().numpy(), calls
    finally:
        model.model.forward = real


@pytest.mark.parametrize("n", [5, 70])
def test_embedding_model_device_tokens_equal_host_tokens(cuda, tmp_path, monkeypatch, n):
    """A written XLM-R directory, python tokeniser on the host side (the library cannot be assumed): the (ids, lens) block of
    every forward call, flagged texts included, and the embeddings' bits."""
    from rag.embedding import EmbeddingModel
    monkeypatch.setenv("CRS_TOKENIZER", "python")
    d = str(tmp_path / "m")
    xc.write_xlmr_dir(d, uc.NFKC_JSON, seed=9, vocab_size=len(uc.vocab()))
    pool = [t for name, t in corpus() if len(t) < 3000]
    flagged = [t for name, t in corpus() if name in uc.FLAGGED and len(t) < 3000]
    texts = (flagged + pool[::2] + pool[1::2])[:n]
    assert len(texts) == n and len(flagged) >= 4
    host = EmbeddingModel({"model_name": d, "batch_size": 32, "tokenize": "host"})
    device = EmbeddingModel({"model_name": d, "batch_size": 32, "tokenize": "device"})
    assert type(device.tokenizer).__name__ == "UnigramTokenizer" and device.shape.pos_offset == 2 and device.shape.max_seq == 64
    emb_h, calls_h = _embed_and_capture(host, texts)
    emb_d, calls_d = _embed_and_capture(device, texts)
    assert type(device._device_tokenizer).__name__ == "UnigramDeviceTokenizer"
    assert len(calls_d) == len(calls_h) == -(-n // 32)
    for b, ((ids_h, lens_h), (ids_d, lens_d)) in enumerate(zip(calls_h, calls_d)):
        assert ids_h.shape == ids_d.shape, (b, ids_h.shape, ids_d.shape)
        assert np.array_equal(lens_h, lens_d), b
        assert np.array_equal(ids_h, ids_d), b
    ids, lens = device.tokenize_device(texts)
    want = host.tokenize(texts)
    assert lens.cpu().numpy().tolist() == [len(w) for w in want]
    got = ids.cpu().numpy()
    for row, w in enumerate(want):
        assert got[row, : len(w)].tolist() == w
    assert np.isfinite(emb_d).all() and np.array_equal(emb_h, emb_d)
