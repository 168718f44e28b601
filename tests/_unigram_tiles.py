"""csrc/unigram.hip's steps 2 and 3 WITH the tiles, in plain Python: what `rag._unigram.table_words` leaves out.  Per tile of
`tile` bytes: the raw elements of the code points whose lead byte lies in the tile, behind what the previous tile carried;
n_proc (how many of them get a role now); what each emits into the word array; whether the tile's end cuts the last word; the
carry; the flag for a word of more than `cap` code points.  tests/test_unigram_tiles_cpu.py holds it to table_words, so a carry rule
that loses or doubles an element shows on the CPU; the GPU tests hold the kernel to the same words' ids."""
from typing import List, Optional

from rag import _native as nat
from rag import _unigram as ug

K_CHAR, K_SP, K_BRK, K_META = ug.K_CHAR, ug.K_SP, ug.K_BRK, ug.K_META
META_CP = ug.META_CP


def _code_point(data: bytes, i: int) -> int:
    """The code point whose lead byte is data[i]; bytes past the end read as 0, as the staged tile's do."""
    b = lambda k: data[i + k] if i + k < len(data) else 0        # noqa: E731
    b0 = data[i]
    if b0 < 0x80:
        return b0
    if b0 < 0xE0:
        return ((b0 & 0x1F) << 6) | (b(1) & 0x3F)
    if b0 < 0xF0:
        return ((b0 & 0x0F) << 12) | ((b(1) & 0x3F) << 6) | (b(2) & 0x3F)
    return ((b0 & 0x07) << 18) | ((b(1) & 0x3F) << 12) | ((b(2) & 0x3F) << 6) | (b(3) & 0x3F)


def tiled_words(text: str, table, opts: int, tile: int, cap: int) -> Optional[List[List[int]]]:
    """The words of `text` (code points, each opening with U+2581) as the kernel's tile loop forms them with tiles of `tile`
    bytes and words of at most `cap` code points; None for a text it flags.  `opts`: the kernel's, CRS_UNIGRAM_CRLF included."""
    collapse, single_meta, run_meta, crlf = (bool(opts & b) for b in (nat.UNIGRAM_COLLAPSE, nat.UNIGRAM_SINGLE_META,
                                                                      nat.UNIGRAM_RUN_META, nat.UNIGRAM_CRLF))
    data = text.encode("utf-8")
    n_bytes = len(data)
    words: List[List[int]] = []
    flagged = False
    carry: List[tuple] = []
    for pos in range(0, n_bytes, tile):
        last_tile = pos + tile >= n_bytes
        # 2. the tile's raw elements behind the carry
        raw = list(carry)
        n_carry = len(carry)
        for i in range(pos, min(pos + tile, n_bytes)):
            if (data[i] & 0xC0) == 0x80:
                continue
            cp = _code_point(data, i)
            if crlf and cp == 0x0D and i + 1 < n_bytes and data[i + 1] == 0x0A:
                continue
            if cp >= len(table.entries):
                flagged = True
                continue
            cls, rep = table.lookup(cp)
            if cls == ug.FALLBACK:
                flagged = True
            elif cls == ug.KEEP:
                raw.extend(rep)
        n_raw = len(raw)
        assert n_raw <= cap + tile + tile // 2 + 32                  # kRaw
        is_sp = [k == K_SP for _, k in raw]

        # 3. roles.  Only where runs collapse does a run of U+0020 at the tile's end wait for the next tile
        last_nonsp = max((i for i in range(n_raw) if not is_sp[i]), default=-1)
        n_proc = n_raw if (last_tile or not collapse) else last_nonsp + 1
        tail_sp = n_raw - n_proc

        def sp_is_meta(i: int) -> bool:
            run = collapse and ((i > 0 and is_sp[i - 1]) or (i + 1 < n_raw and is_sp[i + 1]))
            return run_meta if run else single_meta

        fin: List[int] = []
        for i in range(n_proc):
            cp, kind = raw[i]
            if kind == K_BRK:
                continue
            if kind == K_META:
                fin.append(META_CP)
            elif kind == K_SP:
                if sp_is_meta(i) and not (collapse and i > 0 and is_sp[i - 1]):
                    fin.append(META_CP)
            else:
                if i == 0:
                    after_end = n_carry == 0
                else:
                    pk = raw[i - 1][1]
                    after_end = pk == K_BRK or (pk == K_SP and not sp_is_meta(i - 1))
                if after_end:
                    fin.append(META_CP)
                fin.append(cp)
        last_kind = raw[n_proc - 1][1] if n_proc > 0 else K_BRK
        # a U+0020 ends a tile that is not the last only where runs do not collapse; there it opens a word, as U+2581 itself
        # does, when it stands for a metaspace
        opens = last_kind in (K_CHAR, K_META) or (last_kind == K_SP and single_meta)

        # 4. words: the last one is cut unless the text ends here or something behind it ended it
        starts = [i for i, cp in enumerate(fin) if cp == META_CP]
        cut = (not last_tile) and bool(starts) and tail_sp == 0 and opens
        for k, s in enumerate(starts):
            e = starts[k + 1] if k + 1 < len(starts) else len(fin)
            if e - s > cap:
                flagged = True
            elif not (cut and k == len(starts) - 1):
                words.append(fin[s:e])
        if flagged:
            return None

        carry = []
        if cut:
            w = fin[starts[-1]:]
            carry = [(cp, K_META if k == 0 else K_CHAR) for k, cp in enumerate(w)]
        elif tail_sp > 0:
            carry = [raw[n_proc]] * min(tail_sp, 2)
    return words
