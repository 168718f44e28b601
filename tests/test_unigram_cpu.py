"""CPU: the Unigram tokenisers.  rag.tokenizer.UnigramTokenizer (the restatement) = the `tokenizers` library =
tests/golden/unigram_ids.json.xz id for id; rag._unigram.emulate_encode (the kernel's algorithm on the flat arrays) = the
restatement; the per-code-point table against the tokeniser's own normaliser on random strings; the C boundary."""
import copy
import os
import re

import numpy as np
import pytest

import _unigram_cases as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("nfkc", "spm")
PATHS = {"nfkc": uc.NFKC_JSON, "spm": uc.SPM_JSON}


@pytest.fixture(scope="module")
def golden():
    return uc.load_json(uc.IDS_JSON)


_RESTATED = {}


def restated(kind):
    """The pure-Python tokeniser of a fixture (the Precompiled one needs the library's normaliser object)."""
    if kind not in _RESTATED:
        if kind == "spm":
            pytest.importorskip("tokenizers")
        _RESTATED[kind] = uc.restatement(PATHS[kind])
    return _RESTATED[kind]


_DEVICE_SIDE = {}


def device_side(kind):
    """(spec, table, vocab) of a fixture as the kernel gets them."""
    if kind not in _DEVICE_SIDE:
        from rag import _unigram as ug
        spec = ug.unigram_spec(restated(kind))
        _DEVICE_SIDE[kind] = (spec, ug.table_for_spec(spec), ug.UnigramVocab(spec.pipeline.vocab))
    return _DEVICE_SIDE[kind]


def test_corpus_is_the_committed_one(golden):
    from rag import _native as nat
    assert (golden["cap"], golden["tile"]) == (nat.UNIGRAM_MAX_WORD, nat.UNIGRAM_TILE_BYTES)
    corpus = uc.edge_corpus(nat.UNIGRAM_MAX_WORD, nat.UNIGRAM_TILE_BYTES)
    assert [n for n, _ in corpus] == golden["names"] and [t for _, t in corpus] == golden["texts"]
    assert max(len(t.encode()) for t in golden["texts"]) > 2 * nat.UNIGRAM_TILE_BYTES


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_equals_the_golden_ids(golden, kind):
    tok = restated(kind)
    assert (tok.cls_id, tok.sep_id, tok.pad_id, tok.unk_id) == (0, 2, 1, 3)
    for width in uc.WIDTHS:
        want = golden["ids"][f"{kind}.{width}"]
        for name, text, ids in zip(golden["names"], golden["texts"], want):
            assert tok.encode(text, width) == ids, (kind, width, name)
        assert tok.encode_batch(golden["texts"][:5], width) == want[:5]


@pytest.mark.parametrize("kind", KINDS)
def test_library_equals_the_golden_ids(golden, kind):
    pytest.importorskip("tokenizers")
    tok = uc.library(PATHS[kind])
    for width in uc.WIDTHS:
        assert tok.encode_batch(golden["texts"], width) == golden["ids"][f"{kind}.{width}"], (kind, width)
    full = restated(kind)
    for text in golden["texts"][:40]:
        assert tok.encode_body(text) == full.encode_body(text)
        assert tok.encode(text, 16) == full.encode(text, 16)          # truncation is set again after encode_body


def test_known_pieces_of_the_issue(golden):
    tok = restated("nfkc")
    v = {t: i for i, (t, _) in enumerate(uc.vocab())}
    m = uc.META
    assert tok.encode("ab", 64) == [0, v[m], v["ab"], 2]                              # the tie: the earliest start wins
    assert tok.encode("axyb", 64) == [0, v[m + "a"], 3, v["b"], 2]                    # unknowns in a word fuse
    assert tok.encode("ax yb", 64) == [0, v[m + "a"], 3, v[m], 3, v["b"], 2]          # ... across words they do not
    assert tok.encode("a  b", 64) == tok.encode("a   b", 64) == [0, v[m + "a"], v[m], v["b"], 2]
    assert tok.encode("cd", 64) == [0, v[m], v["c"], v["d"], 2]
    assert tok.encode("   ", 64) == [0, v[m], 2] and tok.encode("", 64) == [0, 2]


@pytest.mark.parametrize("kind", KINDS)
def test_near_tie_flips_under_fp32_sums(kind):
    """`c` + `d` beats `cd` by 3e-8 in fp64.  With fp32 sums the two paths round to one value and the earlier start, `cd`,
    stays: the case can fail."""
    from rag import _unigram as ug
    spec, table, vocab = device_side(kind)
    v = {t: i for i, (t, _) in enumerate(uc.vocab())}
    f32 = lambda a, b: float(np.float32(np.float32(a) + np.float32(b)))      # noqa: E731
    for text, n in (("cd", 1), ("cdcdcd", 3)):
        wrong = ug.emulate_encode(text, table, vocab, spec, 64, add=f32)
        right = ug.emulate_encode(text, table, vocab, spec, 64)
        assert wrong == [0, v[uc.META]] + [v["cd"]] * n + [2]
        assert right == [0, v[uc.META]] + [v["c"], v["d"]] * n + [2] == restated(kind).encode(text, 64)


@pytest.mark.parametrize("kind", KINDS)
def test_emulation_equals_restatement_on_the_edge_corpus(golden, kind):
    from rag import _unigram as ug
    spec, table, vocab = device_side(kind)
    tok = restated(kind)
    flagged = set()
    for name, text in zip(golden["names"], golden["texts"]):
        for width in uc.WIDTHS:
            got = ug.emulate_encode(text, table, vocab, spec, width)
            if got is None:
                flagged.add(name)
            else:
                assert got == tok.encode(text, width), (kind, name, width)
    assert flagged == uc.FLAGGED


@pytest.mark.parametrize("kind", KINDS)
def test_emulation_equals_restatement_on_random_texts(kind):
    """2 000 seeded texts of non-FALLBACK code points; the texts the emulation flags are exactly those with a FALLBACK code point
    or an over-long word (none of the latter here: a text has at most 40 code points)."""
    from rag import _unigram as ug
    spec, table, vocab = device_side(kind)
    tok = restated(kind)
    allowed = np.nonzero(~table.fallback_mask())[0]
    texts = uc.random_texts(2000, 11, allowed)
    fb = table.fallback_mask()
    mixed = uc.random_texts(200, 12, np.arange(0x20, 0x3100))
    n_flagged = 0
    for text in texts + mixed:
        got = ug.emulate_encode(text, table, vocab, spec, 64)
        holds = any(fb[ord(c)] for c in text)
        assert (got is None) == holds, ascii(text)
        n_flagged += got is None
        if got is not None:
            assert got == tok.encode(text, 64), ascii(text)
    assert 0 < n_flagged <= 200


def _strata(rng, n, fb):
    import unicodedata
    ok = np.nonzero(~fb)[0]
    low = ok[ok < 0x3100]
    cf = [cp for cp in range(0x110000) if unicodedata.category(chr(cp)) == "Cf" and not fb[cp]]
    latin = np.asarray([cp for cp in list(range(0x20, 0x250)) + list(range(0x2000, 0x2070)) if not fb[cp]] + cf)
    for pool in (ok, low, latin):
        for _ in range(n):
            yield "".join(map(chr, pool[rng.integers(len(pool), size=24)].tolist()))


@pytest.mark.parametrize("kind", KINDS)
def test_table_concatenation_equals_the_normaliser(kind):
    """The table's soundness: for strings of non-FALLBACK code points, the per-code-point replacements, joined, are what the
    tokeniser's own normaliser (every step but Replace) gives for the whole string; CR LF joined as the table says.  90 000
    random 24-code-point strings in three strata: all code points, below U+3100, Latin + general punctuation + every Cf."""
    from rag import _unigram as ug
    from rag.tokenizer import _library_normalizer
    import unicodedata
    spec, table, _ = device_side(kind)
    if kind == "spm":
        normalize = _library_normalizer(spec.steps).normalize_str
    else:
        normalize = lambda s: unicodedata.normalize("NFKC", s)      # noqa: E731
    fb = table.fallback_mask()
    assert not fb[0x0D] and not fb[0x0A] and table.crlf == (kind == "spm")
    for cp in (0x0301, 0xD55C, 0x200C, 0x200D, 0x1F1E9, 0x1100, 0x1161, 0xE000, 0xFDFA, 0x0378):
        assert fb[cp], hex(cp)
    rep = ["".join(chr(x) for x, _ in table.lookup(cp)[1]) for cp in range(0x110000)]
    rng = np.random.default_rng(5)
    bad = []
    n = 0
    for s in _strata(rng, 30000, fb):
        n += 1
        if n % 50 == 0:                    # CR LF, CR alone and LF alone in a share of the strings
            s = s[:7] + "\r\n" + s[7:15] + "\r" + s[15:20] + "\n\r" + s[20:]
        want = normalize(s)
        got = "".join("" if (table.crlf and c == "\r" and s[i + 1: i + 2] == "\n") else rep[ord(c)] for i, c in enumerate(s))
        if got != want:
            bad.append(ascii(s))
    assert n == 90000 and not bad, bad[:5]


def test_symbols_declared_exported_bound():
    from rag import _native as nat
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crs_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint crs_unigram_encode\s*\(", header), "crs_unigram_encode not declared in include/crs_hip.h"
    for name, want in (("CRS_UNIGRAM_TILE_BYTES", nat.UNIGRAM_TILE_BYTES), ("CRS_UNIGRAM_MAX_WORD", nat.UNIGRAM_MAX_WORD),
                       ("CRS_UNIGRAM_COLLAPSE", nat.UNIGRAM_COLLAPSE), ("CRS_UNIGRAM_SINGLE_META", nat.UNIGRAM_SINGLE_META),
                       ("CRS_UNIGRAM_RUN_META", nat.UNIGRAM_RUN_META), ("CRS_UNIGRAM_CRLF", nat.UNIGRAM_CRLF)):
        m = re.search(rf"#define\s+{name}\s+(\d+)", header)
        assert m and int(m.group(1)) == want, name
    lib = nat.load()
    assert hasattr(lib, "crs_unigram_encode") and "crs_unigram_encode" in nat.exported_symbols()
    assert lib.crs_abi_version() == 3
    assert hasattr(nat.ops(), "unigram_encode") and callable(nat.unigram_encode)
    assert "unigram.hip" in open(os.path.join(ROOT, "compressed-rag-suite_amd", "csrc", "Makefile")).read()


def test_vocabulary_of_xlmr_size_fits_the_table():
    """250 002 pieces: every id and pool offset comes back from the slots (the WordPiece tables never held more than 30 527)."""
    from rag import _unigram as ug
    from rag import _wordpiece as wp
    n = 250002
    vocab = [(f"p{i:x}", -float(i % 97) - i * 1e-9) for i in range(n)]
    uv = ug.UnigramVocab(vocab)
    assert uv.hash.n_entries == n and uv.hash.n_slots == 1 << 19 and uv.slot_scores.dtype == np.float64
    for i in (0, 1, 30527, 65535, 65536, 131071, 200000, n - 1):
        cps = [ord(c) for c in vocab[i][0]]
        assert uv.find(cps, wp.piece_hash(cps, False)) == (i, vocab[i][1])
    assert uv.find([ord("q")], wp.piece_hash([ord("q")], False)) is None


def test_spec_names_what_it_does_not_restate():
    from rag import _unigram as ug
    from rag.tokenizer import UnigramTokenizer
    base = uc.load_json(uc.NFKC_JSON)

    def with_(edit):
        cfg = copy.deepcopy(base)
        edit(cfg)
        return cfg

    with pytest.raises(NotImplementedError, match=r"model\.byte_fallback"):
        UnigramTokenizer(with_(lambda c: c["model"].update(byte_fallback=True)), uc.SPECIAL)
    with pytest.raises(NotImplementedError, match=r"normalizer\[0\]\.type = 'NFD'"):
        UnigramTokenizer(with_(lambda c: c["normalizer"]["normalizers"].__setitem__(0, {"type": "NFD"})), uc.SPECIAL)
    with pytest.raises(NotImplementedError, match=r"pre_tokenizer\.type"):
        UnigramTokenizer(with_(lambda c: c.update(pre_tokenizer={"type": "Whitespace"})), uc.SPECIAL)
    with pytest.raises(NotImplementedError, match=r"post_processor\.type"):
        UnigramTokenizer(with_(lambda c: c.update(post_processor={"type": "RobertaProcessing", "cls": ["<s>", 0], "sep": ["</s>", 2]})), uc.SPECIAL)
    # the older spelling of the prepend scheme is read
    old = with_(lambda c: (c["pre_tokenizer"]["pretokenizers"][1].pop("prepend_scheme"),
                           c["pre_tokenizer"]["pretokenizers"][1].update(add_prefix_space=True)))
    assert UnigramTokenizer(old, uc.SPECIAL).encode("ab", 8) == restated("nfkc").encode("ab", 8)
    # restated on the host, not on the device: a Strip step looks at the whole text
    strip = UnigramTokenizer(with_(lambda c: c["normalizer"]["normalizers"].insert(0, {"type": "Strip", "strip_left": True, "strip_right": True})),
                             uc.SPECIAL)
    assert strip.encode("  ab  ", 8) == restated("nfkc").encode("ab", 8)
    with pytest.raises(NotImplementedError, match=r"tokenize: 'device' .*Strip"):
        ug.unigram_spec(strip)
    assert ug.tokenizer_spec(restated("nfkc")).opts == ug.nat.UNIGRAM_COLLAPSE | ug.nat.UNIGRAM_RUN_META


def test_metaspace_alone_and_lowercase_are_restated():
    """No WhitespaceSplit: a lone U+0020 is a metaspace and other white space stays in the word; the emulation follows."""
    pytest.importorskip("tokenizers")
    from tokenizers import Tokenizer
    from rag import _unigram as ug
    from rag.tokenizer import UnigramTokenizer
    cfg = uc.load_json(uc.NFKC_JSON)
    cfg["pre_tokenizer"] = cfg["pre_tokenizer"]["pretokenizers"][1]
    cfg["normalizer"]["normalizers"].insert(1, {"type": "Lowercase"})
    cfg["normalizer"]["normalizers"][-1]["content"] = " "
    lib = Tokenizer.from_str(__import__("json").dumps(cfg))
    tok = UnigramTokenizer(cfg, uc.SPECIAL)
    spec = ug.unigram_spec(tok)
    table, vocab = ug.table_for_spec(spec), ug.UnigramVocab(spec.pipeline.vocab)
    assert spec.opts == ug.nat.UNIGRAM_COLLAPSE | ug.nat.UNIGRAM_RUN_META | ug.nat.UNIGRAM_SINGLE_META
    for text in ["a b", "a  b", "a ", " a", "  a  ", "a\tb", "", " ", "   ", "The Quick FOX", "a▁b", "ab ab ab", "x  y"]:
        want = lib.encode(text).ids
        assert tok.encode(text, 64) == want, ascii(text)
        assert ug.emulate_encode(text, table, vocab, spec, 64) == want, ascii(text)
