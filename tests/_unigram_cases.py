"""Shared by tools/make_xlmr_golden.py (which writes the Unigram fixtures under tests/golden/ with the `tokenizers` library) and
the Unigram tests: the hand-made vocabulary, the edge corpus, the random texts."""
import json
import lzma
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NFKC_JSON = os.path.join(GOLDEN_DIR, "unigram_nfkc.json")       # normaliser NFKC + Replace(" {2,}", "▁")
SPM_JSON = os.path.join(GOLDEN_DIR, "unigram_spm.json.xz")      # (xz, as enc_plans.json.xz is) normaliser Precompiled(nmt_nfkc) + the same Replace
IDS_JSON = os.path.join(GOLDEN_DIR, "unigram_ids.json.xz")
WIDTHS = (4, 8, 16, 64)
META = "▁"
SPECIAL = {"cls": "<s>", "sep": "</s>", "pad": "<pad>", "unk": "<unk>"}
UNK_ID = 3


def vocab():
    """<s> <pad> </s> <unk>, then at most 200 pieces in all.  `▁ a b ab ▁a` at -1 -1 -1 -2 -2 is the tie of the issue: the three
    paths of `ab` all sum to -3.  `c` + `d` beats `cd` by 3e-8, far below one fp32 ulp of the sums (4.8e-7 at -7): the
    near-tie.  x, y and z are in no piece."""
    v = [("<s>", 0.0), ("<pad>", 0.0), ("</s>", 0.0), ("<unk>", 0.0),
         (META, -1.0), ("a", -1.0), ("b", -1.0), ("ab", -2.0), (META + "a", -2.0),
         ("c", -3.1234567), ("d", -2.7654321), ("cd", -3.1234567 - 2.7654321 - 3e-8)]
    for k, ch in enumerate("efghijklmnopqrstuvw"):
        v.append((ch, -3.5 - 0.013 * k))
    for k, ch in enumerate("ehilmnoprstw"):
        v.append((META + ch, -4.0 - 0.017 * k))
    for k, w in enumerate(["the", "ing", "er", "re", "tion", "ell", "or", "st", "en", "on", "hello", "world", "quick", "fox", "ab" * 8]):
        v.append((w, -5.0 - 0.11 * k))
    for k, w in enumerate(["the", "hello", "world", "to", "of", "in", "is", "fox", "quick", "model", "tokens"]):
        v.append((META + w, -4.5 - 0.07 * k))
    for k, ch in enumerate("0123456789.,!?-'"):
        v.append((ch, -4.2 - 0.009 * k))
    for k, ch in enumerate("ABCEHT"):
        v.append((ch, -6.0 - 0.01 * k))
    for k, ch in enumerate("абвгдеиклмнопрсту"):
        v.append((ch, -5.5 - 0.012 * k))
    for k, w in enumerate([META + "привет", META + "мир", "ир", META + "п", "θ", "é", "ß", "ü",
                           "日", "本", "語", META + "日本", "本語", "中", "文", META + "中"]):
        v.append((w, -6.5 - 0.05 * k))
    v.append(("\u00ad", -9.0))             # a soft hyphen survives nmt_nfkc
    assert len(v) <= 200 and len({t for t, _ in v}) == len(v)
    return v


def filler(n_bytes: int) -> str:
    """Exactly n_bytes of ASCII words, ending in a space."""
    s = ("ab the hello " * (n_bytes // 13 + 1))[: n_bytes - 1]
    return s.rstrip(" ").ljust(n_bytes - 1, "a") + " "


def edge_corpus(cap: int, tile: int):
    """[(name, text)]: the cases of the issue.  `cap`: code points of the longest word the kernel walks, its metaspace included;
    `tile`: bytes staged at a time."""
    out = [("empty", ""), ("spaces", "   "), ("one-space", " "), ("one-char", "a"), ("one-unknown", "x"),
           ("word-cap", "ab" * ((cap - 1) // 2) + "a" * ((cap - 1) % 2)), ("word-cap+1", "ab" * (cap // 2) + "a" * (cap % 2)),
           ("word-cap-after-meta", "a  " + "b" * (cap - 1)), ("word-3cap", "the " + "ab" * (3 * cap // 2) + " fox")]
    for ch, nb in (("é", 2), ("日", 3), ("\U0001d41a", 4)):         # U+1D41A normalises to `a`
        for k in range(1, nb):
            out.append((f"straddle-{nb}byte-{k}", filler(tile - k) + ch + "b the fox"))
        out.append((f"straddle-{nb}byte-0", filler(tile) + ch + "b"))
    for k in range(1, 6):
        out.append((f"straddle-word-{k}", filler(tile - k) + "hello world"))
    out += [("straddle-space-run", filler(tile - 1)[:-1] + "a  b"), ("straddle-space-run-2", filler(tile)[:-1] + "   b"),
            ("straddle-space-single", filler(tile) + " b"), ("straddle-crlf", filler(tile - 1)[:-1] + "a\r\nb"),
            ("two-tiles", "hello world the quick fox ab cd " * (2 * tile // 32 + 3)),
            ("two-tiles-one-word-each", ("ab" * 40 + " ") * 30),
            ("run-2", "a  b"), ("run-3", "a   b"), ("meta-literal", "a\u2581b"), ("meta-lead", "\u2581a"), ("meta-only", "\u2581"),
            ("lead-trail", "  a "), ("trail-1", "a "), ("crlf", "a\r\nb"), ("cr", "a\rb"), ("tab", "a\tb"), ("tab-space", "a \t b"),
            ("nbsp", "a\u00a0b"), ("ideographic-space", "a\u3000b"), ("line-sep", "a\u2028b"), ("zwsp", "a\u200bb"), ("bom", "\ufeffa"),
            ("del", "a\u007fb"), ("soft-hyphen", "a\u00adb"), ("nul", "a\u0000b"),
            ("unknown-inside", "axyb"), ("unknown-across", "ax yb"), ("unknown-only", "xyz xy"), ("unknown-ends", "xay"),
            ("tie", "ab"), ("near-tie", "cd"), ("near-tie-long", "cdcdcd"), ("latin", "The quick fox, hello world!"),
            ("cyrillic", "привет мир"), ("cjk", "日本語 中文"), ("fullwidth", "ＡＢ１"), ("ligature", "ﬁn"), ("sharp-s", "Straße über"),
            ("combining", "e\u0301"), ("hangul", "\ud55c"), ("theta-zwnj", "\u03d1\u200c"), ("flag", "\U0001F1E9\U0001F1EA"),
            ("combining-late", "hello world é"), ("long-replacement", "\ufdfa"),
            ("cut-mid-word", "abxab abxab abxab abxab abxab")]
    return out


FLAGGED = {"word-cap+1", "word-3cap", "combining", "hangul", "theta-zwnj", "flag", "combining-late", "long-replacement"}


def random_texts(n: int, seed: int, allowed: np.ndarray):
    """n texts of 1-40 code points: pieces' own characters and spaces mostly, some drawn from all of `allowed` (code points)."""
    rng = np.random.default_rng(seed)
    common = [ord(c) for c in "abcdefghilmnoprstxyz  \t ▁.,АBпривет日本語中文éßü"]
    common = [c for c in common if c in set(allowed.tolist())]
    out = []
    for _ in range(n):
        k = int(rng.integers(1, 41))
        pick = rng.random(k)
        cps = [common[int(rng.integers(len(common)))] if p < 0.8 else 0x20 if p < 0.9 else int(allowed[int(rng.integers(len(allowed)))])
               for p in pick]
        out.append("".join(map(chr, cps)))
    return out


# ---- tile boundaries and option sets -------------------------------------------------------------------------------------------------
# filler words: 2- and 3-byte characters and two that expand under NFKC, so a byte offset is no element offset
WORDS = ("ab", "the", "hello", "world", "fox", "cd", "é", "über", "привет", "мир", "日本", "中文", "ﬁn", "½", "a½b", "日ﬁ")
UNITS = ([(f"sp{n}", " " * n) for n in (1, 2, 3, 4, 7)]
         + [("tab", "\t"), ("crlf", "\r\n"), ("cr", "\r"), ("lf", "\n"), ("nbsp", "\u00a0"), ("u3000", "\u3000"),
            ("meta", META), ("meta2", META + META), ("2byte", "é"), ("3byte", "日"), ("4byte", "\U0001d41a"),
            ("fi", "ﬁ"), ("half", "½"), ("kabu", "㈱"),                      # 1 code point -> 2, 3, 3
            ("zwsp", "\u200b"), ("del", "\u007f"), ("shy", "\u00ad"),       # nmt_nfkc: a space, dropped, kept
            ("unknown", "x"), ("hello", "hello"), ("world", "world")])
TAIL = "b ab"
DROPPED = "\u007f"          # nmt_nfkc drops it; NFKC keeps it as a character no piece holds


def option_configs():
    """[(name, tokenizer.json dict)]: unigram_nfkc.json edited into every pipeline `rag._unigram.unigram_spec` accepts:
    WhitespaceSplit + Metaspace or Metaspace alone (prepend_scheme always / first), Replace(" {2,}") absent, -> " ", -> "▁"."""
    base = load_json(NFKC_JSON)
    assert [n["type"] for n in base["normalizer"]["normalizers"]] == ["NFKC", "Replace"]
    assert [p["type"] for p in base["pre_tokenizer"]["pretokenizers"]] == ["WhitespaceSplit", "Metaspace"]
    out = []
    for pre in ("split", "alone-always", "alone-first"):
        for rep in (None, " ", META):
            cfg = json.loads(json.dumps(base))
            norms = cfg["normalizer"]["normalizers"]
            if rep is None:
                del norms[1]
            else:
                norms[1]["content"] = rep
            if pre != "split":
                cfg["pre_tokenizer"] = cfg["pre_tokenizer"]["pretokenizers"][1]
                cfg["pre_tokenizer"]["prepend_scheme"] = pre.split("-")[1]
            out.append((f"{pre}.{'none' if rep is None else 'space' if rep == ' ' else 'meta'}", cfg))
    return out


CONFIG_NAMES = tuple(f"{pre}.{rep}" for pre in ("split", "alone-always", "alone-first") for rep in ("none", "space", "meta")) + ("spm",)
# one pipeline per value of the kernel's option bits: 0, COLLAPSE, COLLAPSE|RUN_META, SINGLE_META, all three, and CRLF on top
OPTION_SETS = {"split.none": 0, "split.space": 1, "split.meta": 5, "alone-always.none": 2, "alone-always.meta": 7, "spm": 13}
_SIDES = {}


def config(name):
    """The tokenizer.json dict of a name in CONFIG_NAMES (`spm`: the Precompiled fixture, which needs the `tokenizers` library)."""
    return load_json(SPM_JSON) if name == "spm" else dict(option_configs())[name]


def side(name):
    """(restatement, spec, table, vocabulary, the kernel's opts) of a name in CONFIG_NAMES, built once per process."""
    if name not in _SIDES:
        from rag import _native as nat
        from rag import _unigram as ug
        from rag.tokenizer import UnigramTokenizer
        tok = UnigramTokenizer(config(name), SPECIAL)
        spec = ug.unigram_spec(tok)
        table = ug.table_for_spec(spec)
        _SIDES[name] = (tok, spec, table, ug.UnigramVocab(spec.pipeline.vocab), spec.opts | (nat.UNIGRAM_CRLF if table.crlf else 0))
    return _SIDES[name]


def library_of(name):
    """The `tokenizers` library's own Tokenizer of a name in CONFIG_NAMES, neither padding nor truncating."""
    from tokenizers import Tokenizer
    tok = Tokenizer.from_str(json.dumps(config(name)))
    tok.no_padding()
    tok.no_truncation()
    return tok


def boundary_sweep(tile: int, cap: int):
    """[(name, text)]: every unit at every offset around the first two tile ends, the carried word at cap - 2 .. cap code points
    (`overcap-*`: at cap + 1, which the kernel flags), and the whole-tile cases, each with a third tile behind it."""
    import _tile_cases as tc
    out = tc.sweep(UNITS, WORDS, (tile, 2 * tile), TAIL, seed=31)
    rng = np.random.default_rng(32)
    fill = lambda n, end_space: tc.mixed_filler(n, rng, end_space, WORDS)          # noqa: E731
    for b in (tile, 2 * tile):
        for j in (1, 2, 3):
            for k in (0, 1, 2):                        # cap - k code points with the metaspace in front
                out.append((f"cap-{k}@{b}-{j}", tc.word_at(b, j, cap - 1 - k, WORDS, rng, " ab")))
            out.append((f"overcap-1@{b}-{j}", tc.word_at(b, j, cap, WORDS, rng, " ab")))
    third = lambda: "ab " + fill(tile + tile // 4, True) + "the fox"               # noqa: E731
    out += [("tile-of-spaces", fill(tile, False) + " " * tile + third()),
            ("tile-of-dropped", fill(tile - 2, True) + "he" + DROPPED * tile + "llo " + third()),
            ("tile-ends-in-tab", fill(tile - 1, False) + "\t" + third()),
            ("run-over-two-ends", fill(tile - 3, False) + " " * (tile + 6) + third())]
    assert all(len(t.encode()) > 2 * tile for n, t in out[-4:])
    return out


def sweep_flagged(names, dropped_is_dropped: bool):
    """The names of boundary_sweep the kernel flags: the words over the cap, and the tile of DEL where DEL is a character."""
    return {n for n in names if n.startswith("overcap-")} | (set() if dropped_is_dropped else {"tile-of-dropped"})


def _allowed_units(allowed):
    ok = set(np.asarray(allowed).tolist())
    words = [w for w in WORDS if all(ord(c) in ok for c in w)]
    units = [u for _, u in UNITS if all(ord(c) in ok for c in u)]
    return words, units


def random_long_texts(n: int, seed: int, allowed, cap: int = 128):
    """n texts of 1 to 3.5 KB from WORDS and UNITS (those whose code points are all in `allowed`); no word exceeds `cap`."""
    import _tile_cases as tc
    words, units = _allowed_units(allowed)
    return tc.random_texts(n, seed, words, units, 1024, 3584, cap)


def random_short_texts(n: int, seed: int, allowed):
    """n texts of 4 to 72 bytes from the same alphabet, words of any length: for a tiled model with tiles of 8 to 32 bytes."""
    import _tile_cases as tc
    words, units = _allowed_units(allowed)
    return tc.random_texts(n, seed, words, units, 4, 72, None)


def load_json(path):
    with (lzma.open(path, "rt", encoding="utf-8") if path.endswith(".xz") else open(path, encoding="utf-8")) as fh:
        return json.load(fh)


def restatement(path):
    """rag.tokenizer.UnigramTokenizer of a tokenizer.json fixture."""
    from rag.tokenizer import UnigramTokenizer
    return UnigramTokenizer(load_json(path), SPECIAL)


def library(path):
    """rag.tokenizer.FastUnigramTokenizer of a tokenizer.json fixture (ImportError without the `tokenizers` library)."""
    from tokenizers import Tokenizer
    from rag.tokenizer import FastUnigramTokenizer
    tok = Tokenizer.from_str(json.dumps(load_json(path)))
    tok.no_padding()
    return FastUnigramTokenizer(tok, tok.token_to_id(SPECIAL["cls"]), tok.token_to_id(SPECIAL["sep"]), tok.token_to_id(SPECIAL["pad"]))
