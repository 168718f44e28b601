"""Device tokeniser, host half (rag/_wordpiece.py), no GPU:
  * the per-code-point table restates basic_tokenize exactly outside its FALLBACK set, and that set is small;
  * the vocabulary hash table finds every piece, finds nothing else, and keeps to the probe bound it reports;
  * the kernel's algorithm, run in Python on those two structures, gives WordPieceTokenizer's ids on the edge corpus;
  * the new entry point is declared, exported and bound; the constructor rejects what the device path does not restate."""
import json
import os
import random
import re
import unicodedata

import numpy as np
import pytest

import _wordpiece_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTEXTS = ("ab%scd", "%s", "a%s", "%sb", "a %s b")


def _has_tokenizers():
    try:
        import tokenizers  # noqa: F401
        return True
    except ImportError:
        return False


def _library_tokenizer(lower=True, strip=None):
    from rag.tokenizer import FastWordPieceTokenizer
    return FastWordPieceTokenizer.from_vocab(cases.make_vocab(), lower=lower, strip_accents=strip)


@pytest.mark.parametrize("lower,strip", cases.FLAG_PAIRS)
def test_table_restates_basic_tokenize(lower, strip):
    """Every BMP code point and a seeded 20 000-point sample above it, in five contexts: the words the table gives are the words
    basic_tokenize gives, for every code point the table does not hand to the host."""
    from rag import _wordpiece as wp
    from rag.tokenizer import basic_tokenize
    table = wp.norm_table(lower, strip)
    fallback = table.fallback_mask()
    points = list(range(0x10000)) + random.Random(7).sample(range(0x10000, 0x110000), 20000)
    checked, bad = 0, []
    for cp in points:
        if fallback[cp]:
            continue
        checked += 1
        for ctx in CONTEXTS:
            text = ctx % chr(cp)
            got = wp.table_words(text, table)
            want = basic_tokenize(text, lower, strip)
            if got is None or ["".join(map(chr, w)) for w in got] != want:
                bad.append((hex(cp), ctx))
    assert checked > 55000
    assert not bad, bad[:20]


def test_table_replacements_are_short_and_in_the_pool():
    from rag import _wordpiece as wp
    table = wp.norm_table(True, None)
    ent = table.entries
    n = (ent >> 3) & 3
    offs = (ent >> 8)[n >= 2].astype(np.int64)
    assert offs.min() >= 1 and (offs + n[n >= 2]).max() <= len(table.pool)
    cls, rep, punct = table.lookup(0xD55C)                       # a Hangul syllable: three jamo
    assert cls == wp.KEEP and rep == [0x1112, 0x1161, 0x11AB] and punct == [False] * 3
    assert table.lookup(0x2028)[0] == wp.SPACE and table.lookup(0x4E2D)[0] == wp.ISOLATE and table.lookup(0x200B)[0] == wp.DROP
    assert table.lookup(ord("!"))[2] == [True]
    assert wp.norm_table(True, False).lookup(0x130)[1] == [ord("i"), 0x307]      # accents kept: one code point becomes two


def _assigned_outside_c():
    return [cp for cp in range(0x110000) if unicodedata.category(chr(cp)) not in ("Co", "Cn", "Cs")]


def test_fallback_set_is_small():
    from rag import _wordpiece as wp
    assigned = _assigned_outside_c()
    tables = [wp.norm_table(lower, strip) for lower, strip in cases.FLAG_PAIRS]
    if _has_tokenizers():
        for lower, strip in cases.FLAG_PAIRS:
            tables.append(wp.table_for_spec(wp.tokenizer_spec(_library_tokenizer(lower, strip))))
    for table in tables:
        fb = table.fallback_mask()
        assert fb[0x3A3]
        cats = np.array([unicodedata.category(chr(cp)) in ("Co", "Cn", "Cs") for cp in range(0x110000)])
        assert fb[cats].all()
        assert not fb[:0x250].any()
        assert int(fb[np.asarray(assigned)].sum()) <= len(assigned) // 100


@pytest.mark.skipif(not _has_tokenizers(), reason="the `tokenizers` library is not installed")
def test_library_disagreements_are_real_and_bulk():
    """Each code point the bulk search reports does differ in one of the five contexts when asked one at a time, a sample of the
    others does not, and the search's own time is recorded."""
    from rag import _wordpiece as wp
    from rag.tokenizer import basic_tokenize
    tok = _library_tokenizer()
    table = wp.norm_table(True, None)
    extra, seconds = wp.library_disagreements(tok._tok, table)
    assert seconds < 60 and len(extra) > 0 and extra.min() >= 0x250

    def library_words(text):
        return [w for w, _ in tok._tok.pre_tokenizer.pre_tokenize_str(tok._tok.normalizer.normalize_str(text))]

    for cp in extra[:: max(1, len(extra) // 40)]:
        assert any(library_words(c % chr(cp)) != basic_tokenize(c % chr(cp)) for c in CONTEXTS), hex(cp)
    skip = set(extra.tolist())
    fallback = table.fallback_mask()
    for cp in random.Random(3).sample(range(1, 0x30000), 3000):
        if fallback[cp] or cp in skip:
            continue
        for c in CONTEXTS:
            assert library_words(c % chr(cp)) == basic_tokenize(c % chr(cp)), hex(cp)


def test_vocab_hash_finds_exactly_the_vocabulary():
    from rag import _wordpiece as wp
    vocab = cases.make_vocab()
    vh = wp.VocabHash(vocab)
    assert vh.n_slots >= 2 * vh.n_entries and vh.n_slots & (vh.n_slots - 1) == 0
    assert vh.lmax == max(len(t[2:] if t.startswith("##") and len(t) > 2 else t) for t in vocab)
    for needed in ("##ing", "a", "中", "ᄒ", "##ᅡ", "café"):
        assert needed in vocab
    worst = 0
    for tok, idx in vocab.items():
        cont = tok.startswith("##") and len(tok) > 2
        body = tok[2:] if cont else tok
        count = [0]
        assert vh.lookup([ord(c) for c in body], cont, count=count) == idx, tok
        worst = max(worst, count[0])
    assert worst == vh.max_probe
    rng = random.Random(11)
    alphabet = "abcdefghijklmnopqrstuvwxyzé中ᄒ#"
    for _ in range(3000):
        body = "".join(rng.choice(alphabet) for _ in range(rng.randint(1, 6)))
        cont = rng.random() < 0.5
        count = [0]
        got = vh.lookup([ord(c) for c in body], cont, count=count)
        assert got == vocab.get(("##" if cont else "") + body, -1), (body, cont)
        assert count[0] <= vh.max_probe
    # '##' + body and body are different keys
    assert vh.lookup([ord(c) for c in "ing"], False) == -1 and vh.lookup([ord(c) for c in "ing"], True) == vocab["##ing"]


@pytest.mark.parametrize("lower,strip", cases.FLAG_PAIRS)
def test_emulated_kernel_equals_wordpiece_tokenizer(lower, strip):
    from rag import _wordpiece as wp
    from rag.tokenizer import WordPieceTokenizer
    vocab = cases.make_vocab()
    tok = WordPieceTokenizer(vocab, lower=lower, strip_accents=strip)
    table, vh = wp.norm_table(lower, strip), wp.VocabHash(vocab)
    fast = _library_tokenizer(lower, strip) if _has_tokenizers() else None
    fast_table = wp.table_for_spec(wp.tokenizer_spec(fast)) if fast is not None else None
    n_fallback = 0
    for max_len in (8, 64, 512):
        for text in cases.edge_corpus():
            got = wp.emulate_encode(text, table, max_len, vocab=vh, unk_id=tok.unk_id, cls_id=tok.cls_id, sep_id=tok.sep_id)
            if got is None:
                n_fallback += 1
                assert any(table.lookup(ord(c))[0] == wp.FALLBACK for c in text)
                continue
            assert got == tok.encode(text, max_len), (max_len, text[:60])
            if fast is not None and wp.table_words(text, fast_table) is not None:
                assert got == fast.encode(text, max_len), (max_len, text[:60])
    assert n_fallback == 3 * len(cases.FALLBACK_TEXTS)
    text = cases.megabyte_text()
    assert wp.emulate_encode(text[:4096], table, 16, vocab=vh, unk_id=tok.unk_id, cls_id=tok.cls_id, sep_id=tok.sep_id) == tok.encode(text, 16)


def test_emulated_hash_mode_equals_hash_tokenizer():
    from rag import _wordpiece as wp
    from rag.tokenizer import HashTokenizer
    for size in (30522, 1000):
        tok = HashTokenizer(size)
        spec = wp.tokenizer_spec(tok)
        assert spec.mode == wp.MODE_HASH
        table = wp.table_for_spec(spec)
        for text in cases.edge_corpus():
            got = wp.emulate_encode(text, table, 64, cls_id=spec.cls_id, sep_id=spec.sep_id, hash_lo=spec.hash_lo, hash_span=spec.hash_span)
            if got is not None:
                assert got == tok.encode(text, 64), text[:60]


@pytest.mark.parametrize("lower,strip", cases.FLAG_PAIRS)
def test_boundary_sweep_is_laid_out_and_emulated(lower, strip):
    """What tests/test_wordpiece_tiles_gpu.py launches: every unit stands at its byte offset, the filler in front of it is mixed,
    no text holds a FALLBACK code point, and the emulation (no tiles) gives WordPieceTokenizer's ids for it."""
    from rag import _wordpiece as wp
    from rag.tokenizer import WordPieceTokenizer
    vocab = cases.make_vocab()
    tok = WordPieceTokenizer(vocab, lower=lower, strip_accents=strip)
    table, vh = wp.norm_table(lower, strip), wp.VocabHash(vocab)
    sweep = dict(cases.boundary_sweep())
    assert len(sweep) == len(cases.boundary_sweep()) and 350 <= len(sweep) <= 520
    for label, unit in cases.SWEEP_UNITS:
        nb = len(unit.encode())
        for b in (cases.TILE, 2 * cases.TILE):
            for off in range(b - nb - 2, b + 2):
                t = sweep[f"{label}@{b}{off - b:+d}"].encode()
                assert t[off: off + nb] == unit.encode() and t[off + nb:] == cases.SWEEP_TAIL.encode()
    for b in (cases.TILE, 2 * cases.TILE):
        for j in (1, 2, 3):
            for n in (100, 101):
                t = sweep[f"word-{n}@{b}-{j}"].encode()
                assert t[b - j - 1: b - j + n + 1] == b" " + b"a" * n + b" "
    head = sweep[f"sp3@{2 * cases.TILE}+0"]
    assert {len(c.encode()) for c in head} >= {1, 2, 3} and "한" in head and "İ" in head
    long_texts = cases.random_long_texts()
    sizes = [len(t.encode()) for t in long_texts]
    assert len(long_texts) == 300 and min(sizes) >= 1024 and 3 * 1024 < max(sizes) < 3700
    for text in list(sweep.values()) + list(long_texts[:60]):
        assert not any(table.lookup(ord(c))[0] == wp.FALLBACK for c in set(text))
        got = wp.emulate_encode(text, table, 2048, vocab=vh, unk_id=tok.unk_id, cls_id=tok.cls_id, sep_id=tok.sep_id)
        assert got == tok.encode(text, 2048) and len(got) < 2048, text[-40:]


def test_symbols_declared_exported_bound():
    from rag import _native as nat
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crs_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint crs_wordpiece_encode\s*\(", header), "crs_wordpiece_encode not declared in include/crs_hip.h"
    tile = re.search(r"#define\s+CRS_WORDPIECE_TILE_BYTES\s+(\d+)", header)
    assert tile and int(tile.group(1)) == nat.WORDPIECE_TILE_BYTES == cases.TILE
    lib = nat.load()
    assert hasattr(lib, "crs_wordpiece_encode") and "crs_wordpiece_encode" in nat.exported_symbols()
    assert lib.crs_abi_version() == 3
    assert hasattr(nat.ops(), "wordpiece_encode") and callable(nat.wordpiece_encode)
    src = open(os.path.join(ROOT, "compressed-rag-suite_amd", "csrc", "Makefile")).read()
    assert "wordpiece.hip" in src


def test_bad_tokenize_value_raises():
    from rag.embedding import EmbeddingModel
    for bad in ("gpu", "", None, True):
        with pytest.raises(ValueError, match="tokenize"):
            EmbeddingModel({"model_name": "synthetic:tiny", "tokenize": bad})


@pytest.mark.skipif(not _has_tokenizers(), reason="tokenizer.json needs the `tokenizers` library")
@pytest.mark.parametrize("path,value,field", [
    (("normalizer", "clean_text"), False, "normalizer.clean_text"),
    (("normalizer", "handle_chinese_chars"), False, "normalizer.handle_chinese_chars"),
    (("normalizer",), {"type": "Lowercase"}, "normalizer.type"),
    (("pre_tokenizer",), {"type": "Whitespace"}, "pre_tokenizer.type"),
    (("model", "continuing_subword_prefix"), "@@", "model.continuing_subword_prefix"),
    (("model", "max_input_chars_per_word"), 50, "model.max_input_chars_per_word"),
])
def test_unsupported_tokenizer_json_raises_at_construction(tmp_path, monkeypatch, path, value, field):
    """The constructor itself raises, before any GPU object exists (the GPU check is stubbed out so that this runs anywhere)."""
    from _modeldir import write_model_dir
    from rag import _native as nat
    from rag.embedding import EmbeddingModel
    d = str(tmp_path / "m")
    write_model_dir(d, tokenizer_json=True)
    tj = os.path.join(d, "tokenizer.json")
    cfg = json.load(open(tj, encoding="utf-8"))
    node = cfg
    for key in path[:-1]:
        node = node[key]
    node[path[-1]] = value
    json.dump(cfg, open(tj, "w", encoding="utf-8"))
    monkeypatch.setattr(nat, "require_gpu", lambda: None)
    with pytest.raises(NotImplementedError, match=re.escape(field)):
        EmbeddingModel({"model_name": d, "tokenize": "device"})
    # the same directory under the default setting is none of the device path's business (construction then goes on to the GPU)
    from rag.tokenizer import tokenizer_from_model_dir
    assert tokenizer_from_model_dir(d) is not None


def test_model_that_is_not_wordpiece_raises():
    from rag import _wordpiece as wp

    class Other:
        pass
    with pytest.raises(NotImplementedError):
        wp.tokenizer_spec(Other())
