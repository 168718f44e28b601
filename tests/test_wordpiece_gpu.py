"""Device tokeniser on the GPU (csrc/wordpiece.hip): the ids are the host tokeniser's, id for id.
  * op level: lens, every id and the padding equal WordPieceTokenizer.encode + pad_batch on the edge corpus, at four row widths
    and three flag settings; flags mark exactly the texts with a FALLBACK code point; the hash rule equals HashTokenizer;
  * EmbeddingModel: with rag.embedding.tokenize 'device' every HipEncoder.forward call gets the (ids, lens) block it gets under
    'host', fallback texts included, and the embeddings are then the same bits."""
import os

import numpy as np
import pytest

import _wordpiece_cases as cases

pytestmark = pytest.mark.gpu

_REF = {}


def _reference(lower, strip, max_len):
    """(ids [n, max_len] right-padded, lens [n]) of the edge corpus from WordPieceTokenizer; computed once per setting."""
    key = (lower, strip, max_len)
    if key not in _REF:
        from rag.tokenizer import WordPieceTokenizer, pad_batch
        tok = WordPieceTokenizer(cases.make_vocab(), lower=lower, strip_accents=strip)
        rows, lens = pad_batch([tok.encode(t, max_len) for t in cases.edge_corpus()], tok.pad_id)
        ids = np.full((len(lens), max_len), tok.pad_id, dtype=np.int32)
        ids[:, : rows.shape[1]] = rows
        ids.setflags(write=False)
        lens.setflags(write=False)
        _REF[key] = (ids, lens)
    return _REF[key]


def _device_tokenizer(tok, cuda):
    from rag._wordpiece import DeviceTokenizer
    return DeviceTokenizer(tok, cuda)


def _run(dt, texts, max_len):
    import torch
    ids, lens, flags, host = dt.encode(list(texts), max_len)
    torch.cuda.synchronize()
    assert not host
    return ids.cpu().numpy(), lens.cpu().numpy(), flags.cpu().numpy()


@pytest.mark.parametrize("max_len", [4, 8, 64, 512])
@pytest.mark.parametrize("lower,strip", cases.FLAG_PAIRS)
def test_op_equals_wordpiece_tokenizer(cuda, lower, strip, max_len):
    from rag import _wordpiece as wp
    from rag.tokenizer import WordPieceTokenizer
    tok = WordPieceTokenizer(cases.make_vocab(), lower=lower, strip_accents=strip)
    dt = _device_tokenizer(tok, cuda)
    texts = cases.edge_corpus()
    ids, lens, flags = _run(dt, texts, max_len)
    want_flags = np.array([any(dt.table.lookup(ord(c))[0] == wp.FALLBACK for c in t) for t in texts], dtype=np.int32)
    assert want_flags.sum() == len(cases.FALLBACK_TEXTS)
    assert np.array_equal(flags, want_flags)
    ref_ids, ref_lens = _reference(lower, strip, max_len)
    keep = want_flags == 0
    bad = np.nonzero(keep & (lens != ref_lens))[0]
    assert bad.size == 0, [(int(i), texts[i][:40], int(lens[i]), int(ref_lens[i])) for i in bad[:5]]
    bad = np.nonzero(keep & (ids != ref_ids).any(axis=1))[0]
    assert bad.size == 0, [(int(i), texts[i][:40], ids[i][:12].tolist(), ref_ids[i][:12].tolist()) for i in bad[:5]]


def test_op_reads_a_megabyte_only_as_far_as_it_must(cuda):
    from rag.tokenizer import WordPieceTokenizer
    tok = WordPieceTokenizer(cases.make_vocab())
    dt = _device_tokenizer(tok, cuda)
    texts = [cases.megabyte_text(), "short one", cases.megabyte_text()[3:]]
    ids, lens, flags = _run(dt, texts, 16)
    for row, text in enumerate(texts):
        want = tok.encode(text, 16)
        assert lens[row] == len(want) and ids[row, : len(want)].tolist() == want and (ids[row, len(want):] == tok.pad_id).all()
    assert not flags.any()


@pytest.mark.parametrize("vocab_size", [30522, 1000])
def test_hash_mode_equals_hash_tokenizer(cuda, vocab_size):
    from rag import _wordpiece as wp
    from rag.tokenizer import HashTokenizer
    tok = HashTokenizer(vocab_size)
    dt = _device_tokenizer(tok, cuda)
    texts = cases.edge_corpus()
    for max_len in (8, 64):
        ids, lens, flags = _run(dt, texts, max_len)
        for row, text in enumerate(texts):
            if flags[row]:
                assert any(dt.table.lookup(ord(c))[0] == wp.FALLBACK for c in text)
                continue
            want = tok.encode(text, max_len)
            assert lens[row] == len(want) and ids[row, : len(want)].tolist() == want, (max_len, text[:40])
            assert (ids[row, len(want):] == tok.pad_id).all()
        assert flags.sum() == len(cases.FALLBACK_TEXTS)


def test_two_runs_are_identical(cuda):
    from rag.tokenizer import HashTokenizer, WordPieceTokenizer
    for tok in (WordPieceTokenizer(cases.make_vocab()), HashTokenizer(30522)):
        dt = _device_tokenizer(tok, cuda)
        a = _run(dt, cases.edge_corpus(), 64)
        b = _run(dt, cases.edge_corpus(), 64)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


# ---- EmbeddingModel ------------------------------------------------------------------------------------------------------------------
def _mixed_texts(n):
    corpus = [t for t in cases.edge_corpus() if len(t) < 3000]
    picked = list(cases.FALLBACK_TEXTS) + corpus[::2]
    assert len(picked) >= n
    return picked[:n] if n > 3 else [corpus[1], cases.FALLBACK_TEXTS[0], corpus[-9]]


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


def _check_model(make_model, n):
    texts = _mixed_texts(n)
    host = make_model("host")
    device = make_model("device")
    assert device.tokenize_mode == "device" and host.tokenize_mode == "host"
    emb_h, calls_h = _embed_and_capture(host, texts)
    emb_h2, _ = _embed_and_capture(host, texts)
    emb_d, calls_d = _embed_and_capture(device, texts)
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
    if not np.array_equal(emb_h, emb_h2):
        pytest.skip("two host-path runs of embed_device differ in their bits here, so bit equality of the device path is not asserted")
    assert np.array_equal(emb_h, emb_d)


@pytest.mark.parametrize("n", [3, 200])
@pytest.mark.parametrize("backend", ["python", "library"])
def test_embedding_model_local_dir(cuda, tmp_path, monkeypatch, backend, n):
    from _modeldir import write_model_dir
    from rag.embedding import EmbeddingModel
    if backend == "python":
        monkeypatch.setenv("CRS_TOKENIZER", "python")
    else:
        pytest.importorskip("tokenizers")
    d = str(tmp_path / "m")
    write_model_dir(d, tokenizer_json=(backend == "library"))

    def make(mode):
        m = EmbeddingModel({"model_name": d, "batch_size": 32, "tokenize": mode})
        assert type(m.tokenizer).__name__ == ("WordPieceTokenizer" if backend == "python" else "FastWordPieceTokenizer")
        return m
    _check_model(make, n)
    if backend == "python" and n == 3:       # a lone surrogate has no UTF-8: the text goes to the host tokeniser before the upload
        texts = ["lone \ud800 surrogate", "the quick fox"]
        ids, lens = make("device").tokenize_device(texts)
        want = make("host").tokenize(texts)
        assert lens.cpu().numpy().tolist() == [len(w) for w in want]
        assert all(ids[r, : len(w)].cpu().numpy().tolist() == w for r, w in enumerate(want))


@pytest.mark.parametrize("n", [3, 200])
def test_embedding_model_synthetic_hash(cuda, n):
    from rag.embedding import EmbeddingModel
    _check_model(lambda mode: EmbeddingModel({"model_name": "synthetic:minilm", "batch_size": 32, "tokenize": mode}), n)
