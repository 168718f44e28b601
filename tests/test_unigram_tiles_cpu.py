"""CPU: the Unigram kernel's tile loop and option bits.  tests/_unigram_tiles.py (steps 2-3 with the tiles and the carry) against
`rag._unigram.table_words` (the same steps without tiles) on the boundary sweep at the kernel's tile and on short seeded texts at
tiles of 8, 16 and 32 bytes, for every option set `unigram_spec` can produce; on the sweep also restatement == emulation ==
the `tokenizers` library, for every pipeline of tests/_unigram_cases.option_configs and the Precompiled fixture."""
import numpy as np
import pytest

import _unigram_cases as uc
import _unigram_tiles as ut

_SWEEP = {}


def sweep():
    from rag import _native as nat
    if not _SWEEP:
        _SWEEP["s"] = tuple(uc.boundary_sweep(nat.UNIGRAM_TILE_BYTES, nat.UNIGRAM_MAX_WORD))
    return _SWEEP["s"]


def side(name):
    if name == "spm":
        pytest.importorskip("tokenizers")
    return uc.side(name)


def test_option_configs_reach_every_option_set():
    from rag import _native as nat
    assert (nat.UNIGRAM_COLLAPSE, nat.UNIGRAM_SINGLE_META, nat.UNIGRAM_RUN_META, nat.UNIGRAM_CRLF) == (1, 2, 4, 8)
    names = [n for n, _ in uc.option_configs()]
    assert tuple(names) + ("spm",) == uc.CONFIG_NAMES
    got = {n: uc.side(n)[4] for n in names}
    assert set(got.values()) == {0, 1, 5, 2, 7}
    assert got["alone-first.none"] == got["alone-always.none"] == 2 and got["alone-first.space"] == got["alone-first.meta"] == 7
    pytest.importorskip("tokenizers")
    got["spm"] = side("spm")[4]
    assert got["spm"] == 13
    assert {n: got[n] for n in uc.OPTION_SETS} == uc.OPTION_SETS


def test_the_sweep_is_what_the_issue_lists():
    from rag import _native as nat
    tile, cap = nat.UNIGRAM_TILE_BYTES, nat.UNIGRAM_MAX_WORD
    names = [n for n, _ in sweep()]
    texts = dict(sweep())
    assert len(names) == len(set(names)) and 350 <= len(names) <= 520
    for label, unit in uc.UNITS:
        nb = len(unit.encode())
        for b in (tile, 2 * tile):
            for off in range(b - nb - 2, b + 2):
                t = texts[f"{label}@{b}{off - b:+d}"].encode()
                assert t[off: off + nb] == unit.encode() and t[off + nb:] == uc.TAIL.encode()
    # the filler is mixed: 2- and 3-byte characters and characters that NFKC expands stand in front of the boundary
    head = texts[f"sp3@{2 * tile}+0"]
    assert any(len(c.encode()) == 2 for c in head) and any(len(c.encode()) == 3 for c in head) and "ﬁ" in head and "½" in head
    for b in (tile, 2 * tile):
        for j in (1, 2, 3):
            for k in (0, 1, 2, -1):
                t = texts[f"cap-{k}@{b}-{j}" if k >= 0 else f"overcap-1@{b}-{j}"].encode()
                word = t[b - j:].split(b" ")[0]
                assert t[b - j - 1: b - j] == b" " and len(word) == cap - 1 - k and word.isalpha()
    sp = texts["tile-of-spaces"].encode()
    assert sp[tile - 1: 2 * tile + 1] == b"b" + b" " * tile + b"a"
    dr = texts["tile-of-dropped"].encode()
    assert dr[tile - 3: 2 * tile + 1] == b" he" + b"\x7f" * tile + b"l"
    assert texts["tile-ends-in-tab"].encode()[tile - 2: tile + 1] == b"b\ta"
    run = texts["run-over-two-ends"].encode()
    assert run[tile - 4: 2 * tile + 4] == b"b" + b" " * (tile + 6) + b"a"


@pytest.mark.parametrize("name", uc.CONFIG_NAMES)
def test_tiles_restatement_emulation_library_agree_on_the_sweep(name, monkeypatch):
    """For every text of the sweep: the tiled model at the kernel's tile and cap gives table_words' words (None exactly for the
    words over the cap), the emulation gives the restatement's ids, and the restatement gives the library's.  The fillers repeat
    their words, so emulate_encode's walk of one word is remembered per word: 6 s of walks become half a second."""
    pytest.importorskip("tokenizers")
    from rag import _native as nat
    from rag import _unigram as ug
    tok, spec, table, vocab, opts = side(name)
    walk, seen = ug.emulate_word, {}

    def remembered(w, *args, **kwargs):
        key = tuple(w)
        if key not in seen:
            seen[key] = walk(w, *args, **kwargs)
        return list(seen[key])

    monkeypatch.setattr(ug, "emulate_word", remembered)
    lib = uc.library_of(name)
    tile, cap = nat.UNIGRAM_TILE_BYTES, nat.UNIGRAM_MAX_WORD
    assert not any(table.lookup(ord(c))[0] == ug.FALLBACK for c in "".join(uc.WORDS) + "".join(u for _, u in uc.UNITS) + uc.TAIL)
    flagged = set()
    for case, text in sweep():
        words = ug.table_words(text, table, spec.opts)
        assert words is not None, (name, case)
        tiled = ut.tiled_words(text, table, opts, tile, cap)
        if any(len(w) > cap for w in words):
            flagged.add(case)
            assert tiled is None, (name, case)
        else:
            assert tiled == words, (name, case)
        want = tok.encode(text, 4096)
        assert len(want) < 4096
        assert want[1:-1] == lib.encode(text, add_special_tokens=False).ids, (name, case)
        emu = ug.emulate_encode(text, table, vocab, spec, 4096)
        assert (emu is None) == (case in flagged) and (emu is None or emu == want), (name, case)
    assert flagged == uc.sweep_flagged([n for n, _ in sweep()], table.lookup(ord(uc.DROPPED))[0] == ug.DROP)


@pytest.mark.parametrize("name", tuple(uc.OPTION_SETS))
def test_tiled_model_equals_table_words_at_small_tiles(name):
    """6 000 seeded texts of 4 to 72 bytes per (tile, cap): at 8, 16 and 32 bytes nearly every text crosses several tile ends,
    in every state the carry can be in; at caps 6 and 8 the carried word meets its cap as well."""
    from rag import _unigram as ug
    tok, spec, table, vocab, opts = side(name)
    allowed = np.nonzero(~table.fallback_mask())[0]
    texts = uc.random_short_texts(6000, 41, allowed)
    untiled = [ug.table_words(t, table, spec.opts) for t in texts]
    assert all(w is not None for w in untiled)
    for tile, cap in ((8, 6), (16, 8), (32, 128)):
        n_flagged = 0
        for text, words in zip(texts, untiled):
            want = None if any(len(w) > cap for w in words) else words
            assert ut.tiled_words(text, table, opts, tile, cap) == want, (name, tile, cap, ascii(text))
            n_flagged += want is None
        assert (n_flagged == 0) == (cap == 128) and len(texts) - n_flagged >= 500


@pytest.mark.parametrize("name", tuple(uc.OPTION_SETS))
def test_random_long_texts_are_not_flagged(name):
    """What the GPU test launches: 300 texts of 1 to 3.5 KB, none flagged, the tiled model and the emulation agreeing on a sample."""
    from rag import _native as nat
    from rag import _unigram as ug
    tok, spec, table, vocab, opts = side(name)
    allowed = np.nonzero(~table.fallback_mask())[0]
    texts = uc.random_long_texts(300, 51, allowed)
    sizes = [len(t.encode()) for t in texts]
    assert min(sizes) >= 1024 and max(sizes) > 3 * 1024 and max(sizes) < 3700
    for text in texts[:60]:
        words = ug.table_words(text, table, spec.opts)
        assert words is not None and max(len(w) for w in words) <= nat.UNIGRAM_MAX_WORD
        assert ut.tiled_words(text, table, opts, nat.UNIGRAM_TILE_BYTES, nat.UNIGRAM_MAX_WORD) == words, ascii(text[:60])
