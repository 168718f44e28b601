"""Shared by tests/_unigram_cases.py and tests/_wordpiece_cases.py: texts that put a unit at every byte offset around a tile
boundary of the device tokenisers (csrc/unigram.hip and csrc/wordpiece.hip walk a text in tiles of 1024 bytes), behind a filler
whose byte offsets and element offsets differ, and seeded texts of several tiles.  Everything is a function of its arguments."""
import numpy as np


def mixed_filler(n_bytes: int, rng, end_space: bool, words) -> str:
    """Exactly n_bytes of UTF-8: `words` drawn by `rng` with one U+0020 between them, then at most 17 bytes of ASCII that end in
    a space (end_space) or in a letter, so that what follows continues a word."""
    if n_bytes <= 0:
        return ""
    parts, left = [], n_bytes
    while left > 17:
        w = words[int(rng.integers(len(words)))]
        nb = len(w.encode()) + 1
        if nb > left - 1:
            break
        parts.append(w + " ")
        left -= nb
    return "".join(parts) + "a" * (left - 1) + (" " if end_space else "b")


def sweep(units, words, boundaries, tail: str, seed: int):
    """[(name, text)]: for every boundary B and every (label, unit), the unit's first byte at each offset from
    B - len(unit) - 2 to B + 1, behind a mixed filler that ends in a letter or in a space (drawn), with `tail` behind it."""
    rng = np.random.default_rng(seed)
    out = []
    for b in boundaries:
        for label, unit in units:
            nb = len(unit.encode())
            for off in range(b - nb - 2, b + 2):
                text = mixed_filler(off, rng, bool(rng.integers(2)), words) + unit + tail
                assert len(text.encode()) == off + nb + len(tail.encode())
                out.append((f"{label}@{b}{off - b:+d}", text))
    return out


def word_at(b: int, j: int, n_chars: int, words, rng, tail: str, letters: str = "ab") -> str:
    """A word of n_chars ASCII letters (`letters` repeated) that starts at byte b - j, a space in front of it."""
    return mixed_filler(b - j, rng, True, words) + (letters * n_chars)[:n_chars] + tail


def random_texts(n: int, seed: int, words, units, lo_bytes: int, hi_bytes: int, cap, expands: int = 3):
    """n texts of lo_bytes to hi_bytes bytes (a unit may overshoot): words half of the time, a single U+0020 a quarter, any
    unit otherwise.  With `cap`, a U+0020 is put in before the code points since the last U+0020 (each counted `expands`
    times: what a normaliser can make of one) could exceed cap - 2, so no word is longer than cap whatever ends words."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        target = int(rng.integers(lo_bytes, hi_bytes + 1))
        parts, n_b, run = [], 0, 0
        while n_b < target:
            p = rng.random()
            u = words[int(rng.integers(len(words)))] if p < 0.5 else " " if p < 0.75 else units[int(rng.integers(len(units)))]
            if set(u) == {" "}:
                run = 0
            else:
                if cap is not None and run + expands * len(u) > cap - 2:
                    parts.append(" ")
                    n_b += 1
                    run = 0
                run += expands * len(u)
            parts.append(u)
            n_b += len(u.encode())
        out.append("".join(parts))
    return out
