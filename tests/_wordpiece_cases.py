"""Shared by tests/test_wordpiece_cpu.py and tests/test_wordpiece_gpu.py: a test vocabulary and the edge corpus of the device
tokeniser (csrc/wordpiece.hip).  The corpus is built once per process and never changed."""
import functools
import random

from _modeldir import make_vocab as _base_vocab

TILE = 1024          # rag._native.WORDPIECE_TILE_BYTES; test_wordpiece_cpu.py holds the two (and the header) together
FLAG_PAIRS = ((True, None), (True, False), (False, False))
FALLBACK_TEXTS = ("alpha \u03a3 beta", "private \ue000 use", "unassigned \u0378 point")


def make_vocab():
    """_modeldir's vocabulary plus what the device tokeniser's corners need: '#', a CJK character, Hangul jamo (what NFD makes of a
    syllable), accented pieces (reachable only when accents are kept), upper case (reachable only when case is kept)."""
    extra = ["#", "\u4e2d", "\u6587", "\u1112", "##\u1161", "##\u11ab", "\u1100", "##\u116e", "##\u11a8", "caf\u00e9", "\u00e9",
             "##\u00e9", "na", "##\u00ef", "##ve", "i\u0307", "The", "FOX", "A", "##B", "\u00fc", "##\u00fc", "ber", "(", ")", "\u3002",
             "##\u0307", "jump", "fox", "##es", "##ization", "token"]
    out = _base_vocab()
    seen = set(out)
    for t in extra:
        if t not in seen:
            seen.add(t)
            out.append(t)
    return {t: i for i, t in enumerate(out)}


def _straddle(unit: str, boundary: int, delta: int, word: str = "retrieval ") -> str:
    """ASCII words up to `boundary + delta` bytes, then `unit` (so its first byte sits at that offset), then a tail."""
    body = (word * (boundary // len(word) + 2))[: boundary + delta]
    return body + unit + " tail of the text"


@functools.lru_cache(maxsize=None)
def edge_corpus():
    """About 300 seeded short texts and the hand-made corners; a tuple of str."""
    rng = random.Random(20240611)
    vocab_words = [w for w in _base_vocab() if w.isalpha() and len(w) > 1]
    bits = vocab_words + ["caf\u00e9", "na\u00efve", "\u00dcber", "\u0130stanbul", "\u4e2d\u6587", "\ud55c\uad6d\uc5b4", "!", "...", "##",
                          "-", "'s", " ", "\t", "  ", "\u00a0", "\u200b", "\x00", "\u00f1", "\u00df", "\u00c5", "\u01c6", "The", "FOX",
                          "42", "3.14", "e\u0301", "\u3002", "(", ")", "\ufffd", "\U0001f600", "unknownword", "xyzzy", "tokenization",
                          "foxes", "\u2028", "\u3000"]
    texts = []
    for _ in range(300):
        n = rng.randint(1, 12)
        texts.append("".join(rng.choice(bits) + rng.choice(("", " ", " ", " ")) for _ in range(n)))
    texts += [
        "", "   \t\n  ", "\x00\u200b\ufffd\x07", "   leading and trailing   ", "!!!...???,,,--", "## ##ing a##b #", "a" * 100, "a" * 101,
        "x " + "a" * 100 + " y " + "a" * 101 + " z", "b" * 5000, "the " + "q" * 5000 + " fox", "caf\u00e9 \u0130 r\u00e9sum\u00e9 na\u00efve",
        "abc\u4e2d\u6587def\u4e2dg", "line\u2028separator\u2029paragraph", "the qu\u00a4ck brown", "over zzzqzzz lazy", "dogs foxes jumpsing",
        "\ud55c\uad6d\uc5b4 \ud55c", "\u01fa \u1eb9\u0301",
    ]
    for boundary in (TILE, 2 * TILE):
        for delta in (-1, 0, 1):
            texts.append(_straddle("augmented", boundary, delta - 4))            # an ASCII word across the boundary
            for unit in ("\u00e9", "\u4e2d", "\U0001f600", "\ud55c\uad6d"):       # 2-, 3-, 4-byte characters; Hangul 1 -> 3
                for k in range(len(unit[0].encode("utf-8"))):
                    texts.append(_straddle(unit, boundary, delta - k))
    # token counts around the cut: single-token words, then a three-piece word (jumps ##ing ##s) where the row ends
    for max_len in (4, 8, 64, 512):
        for short in range(0, 5):
            texts.append("the " * max(0, max_len - 2 - short) + "jumpsings foxes")
    texts += list(FALLBACK_TEXTS)
    return tuple(texts)


# ---- tile boundaries ----------------------------------------------------------------------------------------------------------------
# filler words: 2- and 3-byte characters, CJK (a word of its own per character), Hangul and U+0130 (one code point -> three / two
# elements), so a byte offset is no element offset
SWEEP_WORDS = ("retrieval", "augmented", "the", "fox", "jumpsing", "café", "naïve", "Über", "İstanbul", "中文",
               "한국어", "tokenization", "a", "xyzzy", "3.14", "FOX")
SWEEP_UNITS = (("sp1", " "), ("sp2", "  "), ("sp3", "   "), ("tab", "\t"), ("crlf", "\r\n"), ("nbsp", "\u00a0"), ("u3000", "\u3000"),
               ("2byte", "\u00e9"), ("3byte", "\u4e2d"), ("4byte", "\U0001f600"), ("hangul", "\ud55c"), ("hangul2", "\ud55c\uad6d"),
               ("dotted-i", "\u0130"), ("dz", "\u01c6"), ("sharp-s", "\u00df"), ("combining", "e\u0301"), ("punct", "!"), ("dots", "..."),
               ("hashes", "##"), ("cjk-stop", "\u3002"), ("zwsp", "\u200b"), ("nul", "\x00"), ("replacement", "\ufffd"),
               ("word", "augmented"), ("pieces", "foxes"), ("unknown", "xyzzy"))
SWEEP_TAIL = "b tail"


@functools.lru_cache(maxsize=None)
def boundary_sweep():
    """(name, text) pairs: every unit of SWEEP_UNITS with its first byte at every offset from B - len(unit) - 2 to B + 1 for B in
    (TILE, 2 * TILE) behind a mixed filler, and a word of 100 and of 101 characters (max_input_chars_per_word is 100) that starts
    1 to 3 bytes in front of B."""
    import numpy as np
    import _tile_cases as tc
    out = tc.sweep(SWEEP_UNITS, SWEEP_WORDS, (TILE, 2 * TILE), SWEEP_TAIL, seed=61)
    rng = np.random.default_rng(62)
    for b in (TILE, 2 * TILE):
        for j in (1, 2, 3):
            for n in (100, 101):
                out.append((f"word-{n}@{b}-{j}", tc.word_at(b, j, n, SWEEP_WORDS, rng, " tail of the text", letters="a")))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def random_long_texts(n: int = 300, seed: int = 63):
    """n seeded texts of 1 to 3.5 KB from SWEEP_WORDS and SWEEP_UNITS, no word of more than 100 elements (a code point counts as the
    three elements a Hangul syllable becomes)."""
    import _tile_cases as tc
    return tuple(tc.random_texts(n, seed, SWEEP_WORDS, [u for _, u in SWEEP_UNITS], 1024, 3584, 100))


@functools.lru_cache(maxsize=None)
def megabyte_text():
    return ("retrieval augmented generation embeds chunks of text, " * 20000)[: 1 << 20]
