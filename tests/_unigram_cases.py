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
