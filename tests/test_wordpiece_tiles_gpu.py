"""GPU: crs_wordpiece_encode (csrc/wordpiece.hip) across tile boundaries.  The boundary sweep of tests/_wordpiece_cases.py (every
unit at every byte offset around the first two tile ends behind a mixed filler, words of 100 and 101 characters that start just
in front of a tile end) and 300 seeded texts of 1 to 3.5 KB: lens, every id and the padding equal WordPieceTokenizer.encode for
the three flag settings at a row the budget ends early in and at one that holds every id, and HashTokenizer.encode; no text is
flagged, and the test asserts before the launch that none holds a FALLBACK code point."""
import numpy as np
import pytest

import _wordpiece_cases as cases

pytestmark = pytest.mark.gpu


def _texts():
    return [t for _, t in cases.boundary_sweep()] + list(cases.random_long_texts())


def _names():
    return [n for n, _ in cases.boundary_sweep()] + [f"random-{i}" for i in range(len(cases.random_long_texts()))]


def _check(tok, cuda, max_len):
    import torch
    from rag import _wordpiece as wp
    dt = wp.DeviceTokenizer(tok, cuda)
    texts, names = _texts(), _names()
    fallback = {c for c in set("".join(texts)) if dt.table.lookup(ord(c))[0] == wp.FALLBACK}
    assert not fallback, sorted(map(hex, map(ord, fallback)))
    ids, lens, flags, host = dt.encode(texts, max_len)
    torch.cuda.synchronize()
    assert not host
    ids, lens, flags = ids.cpu().numpy(), lens.cpu().numpy(), flags.cpu().numpy()
    assert ids.shape == (len(texts), max_len) and not flags.any()
    bad = []
    for r, (name, text) in enumerate(zip(names, texts)):
        want = tok.encode(text, max_len)
        if lens[r] != len(want):
            bad.append((name, "lens", int(lens[r]), len(want)))
        elif ids[r, : lens[r]].tolist() != want:
            k = int(np.nonzero(ids[r, : lens[r]] != np.asarray(want))[0][0])
            bad.append((name, "id", k, ids[r, k: k + 4].tolist(), want[k: k + 4]))
        elif not (ids[r, lens[r]:] == tok.pad_id).all():
            bad.append((name, "padding"))
    assert not bad, (max_len, len(bad), bad[:12])
    return ids, lens, names


@pytest.mark.parametrize("max_len", [64, 2048])
@pytest.mark.parametrize("lower,strip", cases.FLAG_PAIRS)
def test_sweep_and_long_texts_equal_wordpiece_tokenizer(cuda, lower, strip, max_len):
    from rag.tokenizer import WordPieceTokenizer
    tok = WordPieceTokenizer(cases.make_vocab(), lower=lower, strip_accents=strip)
    ids, lens, names = _check(tok, cuda, max_len)
    if max_len == 2048:        # no row fills: the word of 100 characters is 100 pieces, the word of 101 one [UNK], on both sides of a cut
        assert lens.max() < 2048
        for b in (cases.TILE, 2 * cases.TILE):
            for j in (1, 2, 3):
                r100, r101 = names.index(f"word-100@{b}-{j}"), names.index(f"word-101@{b}-{j}")
                tail = len(tok.encode(" tail of the text", 64)) - 1
                assert (ids[r100, lens[r100] - tail - 100: lens[r100] - tail] != tok.unk_id).all()
                assert ids[r101, lens[r101] - tail - 1] == tok.unk_id


def test_sweep_and_long_texts_equal_hash_tokenizer(cuda):
    from rag.tokenizer import HashTokenizer
    _check(HashTokenizer(30522), cuda, 2048)
