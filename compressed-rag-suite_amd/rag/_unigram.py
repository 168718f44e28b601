"""Host side of the device Unigram tokeniser (csrc/unigram.hip, `rag.embedding.tokenize: 'device'` with an XLM-RoBERTa model).

Built here, from what `rag.tokenizer.unigram_pipeline` reads out of tokenizer.json, and handed to the kernel as flat arrays:

* ``unigram_norm_table``: every normaliser step but Replace(" {2,}") as ONE uint32 per code point -- DROP, KEEP with a replacement
  of one to three code points (each with a kind: character, U+0020, other white space, U+2581), or FALLBACK.  The entries come
  from calling the tokeniser's own normaliser on each code point; that is sound only where the normaliser looks at no
  neighbour, so every code point that can join a grapheme cluster or compose with its neighbour is FALLBACK.
* the vocabulary as `rag._wordpiece.VocabHash` (no continuation bit) plus one fp64 score per slot.
* ``emulate_encode``: the kernel's algorithm in plain Python on those arrays (tests/test_unigram_cpu.py holds it to
  `UnigramTokenizer.encode`; the kernel is held to the same ids on the GPU).

``device_tokenizer`` / ``tokenizer_spec`` pick this module or rag/_wordpiece.py by the tokeniser's type.
"""
from __future__ import annotations

import json
import re
import time
import unicodedata
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from rag import _native as nat
from rag import _wordpiece as wp
from rag.tokenizer import (META, RUST_WHITESPACE, UNK_PENALTY, FastUnigramTokenizer, UnigramPipeline, UnigramTokenizer,
                           _library_normalizer, unigram_pipeline)

DROP, KEEP, FALLBACK = 0, 3, 4
K_CHAR, K_SP, K_BRK, K_META = 0, 1, 2, 3
N_CODE_POINTS = 0x110000
MAX_WORD = nat.UNIGRAM_MAX_WORD
META_CP = ord(META)

# table entry: bits 0-2 class | bits 3-4 replacement length n | bits 5-10 kind of each replacement code point (2 bits each) |
# bits 11-31: n == 1: the code point; n >= 2: offset of the n code points in the replacement pool
_CLS_MASK, _N_SHIFT, _K_SHIFT, _V_SHIFT = 7, 3, 5, 11

# code points that take part in a grapheme cluster with a neighbour (the Precompiled normaliser maps cluster by cluster) or
# compose with one under NFC / NFKC, listed for a Python without the `regex` module; with it, \p{GCB} decides as well
_CLUSTER_RANGES = ((0x1100, 0x11FF), (0xA960, 0xA97F), (0xAC00, 0xD7FF),      # Hangul jamo L / V / T and syllables LV / LVT
                   (0x200C, 0x200D), (0x1F1E6, 0x1F1FF), (0x1F3FB, 0x1F3FF), (0xE0000, 0xE0FFF),   # ZWNJ ZWJ, flags, skin tones, tags
                   (0x0600, 0x0605), (0x06DD, 0x06DD), (0x070F, 0x070F), (0x0890, 0x0891), (0x08E2, 0x08E2), (0x0D4E, 0x0D4E),
                   (0x110BD, 0x110BD), (0x110CD, 0x110CD), (0xFF9E, 0xFF9F))                          # Prepend; halfwidth voicing marks


def contextual_code_points() -> np.ndarray:
    """bool [0x110000]: True where a per-code-point table cannot restate the normaliser."""
    ctx = np.zeros(N_CODE_POINTS, dtype=bool)
    cat = unicodedata.category
    for cp in range(N_CODE_POINTS):
        c = cat(chr(cp))
        if c in ("Mn", "Mc", "Me", "Cn", "Co", "Cs") or unicodedata.combining(chr(cp)):
            ctx[cp] = True
    for lo, hi in _CLUSTER_RANGES:
        ctx[lo: hi + 1] = True
    try:
        import regex
    except ImportError:
        return ctx
    plain = regex.compile(r"[\p{GCB=Other}\p{GCB=Control}\p{GCB=CR}\p{GCB=LF}]")
    for cp in range(N_CODE_POINTS):
        if not ctx[cp] and not plain.match(chr(cp)):
            ctx[cp] = True
    return ctx


class UnigramTable:
    """entries uint32 [0x110000], pool uint32 [m] (m >= 1), crlf: CR LF gives what LF alone gives."""

    def __init__(self, entries: np.ndarray, pool: np.ndarray, crlf: bool, build_seconds: float):
        self.entries, self.pool, self.crlf, self.build_seconds = entries, pool, crlf, build_seconds
        self._list = None

    def lookup(self, cp: int) -> Tuple[int, List[Tuple[int, int]]]:
        """(class, [(code point, kind)])"""
        if self._list is None:
            self._list = self.entries.tolist()
        e = self._list[cp]
        n, v = (e >> _N_SHIFT) & 3, e >> _V_SHIFT
        rep = [] if n == 0 else [v] if n == 1 else [int(x) for x in self.pool[v: v + n]]
        return e & _CLS_MASK, [(x, (e >> (_K_SHIFT + 2 * i)) & 3) for i, x in enumerate(rep)]

    def fallback_mask(self) -> np.ndarray:
        return (self.entries & _CLS_MASK) == FALLBACK


def unigram_norm_table(normalize: Callable[[str], str], ws_split: bool) -> UnigramTable:
    """`normalize` (every step of the tokeniser's normaliser except Replace) on each code point, as the kernel's table."""
    t0 = time.perf_counter()
    ent = np.zeros(N_CODE_POINTS, dtype=np.uint32)
    ctx = contextual_code_points()
    pool: List[int] = [0]
    for cp in range(N_CODE_POINTS):
        if ctx[cp]:
            ent[cp] = FALLBACK
            continue
        rep = normalize(chr(cp))
        n = len(rep)
        if n > 3:
            ent[cp] = FALLBACK
            continue
        if n == 0:
            ent[cp] = DROP
            continue
        bits = KEEP | (n << _N_SHIFT)
        for i, x in enumerate(rep):
            o = ord(x)
            kind = K_SP if o == 0x20 else K_META if o == META_CP else K_BRK if (ws_split and o in RUST_WHITESPACE) else K_CHAR
            bits |= kind << (_K_SHIFT + 2 * i)
        if n == 1:
            ent[cp] = bits | (ord(rep) << _V_SHIFT)
        else:
            ent[cp] = bits | (len(pool) << _V_SHIFT)
            pool.extend(ord(x) for x in rep)
    crlf = normalize("\r\n") != normalize("\r") + normalize("\n")
    if crlf and normalize("\r\n") != normalize("\n"):      # joined into something else: leave CR to the host
        ent[0x0D], crlf = FALLBACK, False
    return UnigramTable(ent, np.asarray(pool, dtype=np.uint32), crlf, time.perf_counter() - t0)


# ---- what a tokeniser object asks of the kernel ------------------------------------------------------------------------------------
class UnigramSpec:
    def __init__(self, pipeline: UnigramPipeline, opts: int, cls_id: int, sep_id: int, pad_id: int, library=None):
        self.pipeline, self.opts, self.cls_id, self.sep_id, self.pad_id, self.library = pipeline, opts, cls_id, sep_id, pad_id, library
        self.unk_id = pipeline.unk_id
        self.unk_score = min(sc for _, sc in pipeline.vocab) - UNK_PENALTY
        self.added = tuple(a["content"] for a in pipeline.added)
        self.steps = tuple(st for st in pipeline.steps if st[0] != "replace")


def _require(cond: bool, field: str, got) -> None:
    if not cond:
        raise NotImplementedError(f"tokenize: 'device' does not restate this tokenizer: {field} = {got!r}")


def unigram_spec(tok) -> UnigramSpec:
    """What a UnigramTokenizer / FastUnigramTokenizer computes, as the kernel's arguments; NotImplementedError, naming the field,
    for a setting the device path does not restate (a Strip step looks at the whole text; Replace must come last)."""
    if isinstance(tok, FastUnigramTokenizer):
        p, library = unigram_pipeline(json.loads(tok._tok.to_str())), tok._tok
    else:
        p, library = tok.pipeline, None
    kinds = [st[0] for st in p.steps]
    _require("strip" not in kinds, "normalizer.type", "Strip")
    _require(kinds.count("replace") <= 1 and "replace" not in kinds[:-1], "normalizer (Replace must be the last step)", kinds)
    _require(p.prepend == "always" or (p.prepend == "first" and not p.ws_split), "pre_tokenizer.prepend_scheme", p.prepend)
    opts = 0
    if "replace" in kinds:
        opts |= nat.UNIGRAM_COLLAPSE
        if not p.ws_split or p.steps[-1][2] == META:
            opts |= nat.UNIGRAM_RUN_META
    if not p.ws_split:
        opts |= nat.UNIGRAM_SINGLE_META
    return UnigramSpec(p, opts, tok.cls_id, tok.sep_id, tok.pad_id, library)


def is_unigram(tok) -> bool:
    return isinstance(tok, (UnigramTokenizer, FastUnigramTokenizer))


def tokenizer_spec(tok):
    """unigram_spec or rag._wordpiece.tokenizer_spec, by the tokeniser's type."""
    return unigram_spec(tok) if is_unigram(tok) else wp.tokenizer_spec(tok)


_table_cache: Dict[tuple, UnigramTable] = {}


def table_for_spec(spec: UnigramSpec) -> UnigramTable:
    """Built once per process and normaliser (about a second with the library's normaliser, a few with unicodedata)."""
    key = (json.dumps(spec.steps), spec.pipeline.ws_split, spec.library is not None)
    if key not in _table_cache:
        if spec.library is not None or any(st[0] == "precompiled" for st in spec.steps):
            normalize = _library_normalizer(spec.steps).normalize_str       # ImportError without the library: Precompiled needs it
        else:
            def normalize(s, steps=spec.steps):
                for st in steps:
                    s = s.lower() if st[0] == "lower" else unicodedata.normalize("NFKC" if st[0] == "nfkc" else "NFC", s)
                return s
        _table_cache[key] = unigram_norm_table(normalize, spec.pipeline.ws_split)
    return _table_cache[key]


class UnigramVocab:
    """The pieces as a VocabHash (no continuation bit) and the fp64 score of the piece in each slot."""

    def __init__(self, vocab: Sequence[Tuple[str, float]]):
        ids = {t: i for i, (t, _) in enumerate(vocab) if 0 < len(t) <= MAX_WORD}      # a repeated piece keeps its last id
        self.hash = wp.VocabHash(ids, prefix=None)
        by_id = np.asarray([sc for _, sc in vocab], dtype=np.float64)
        slots = self.hash.slots
        self.slot_scores = np.zeros(self.hash.n_slots, dtype=np.float64)
        used = slots[:, 1] != 0
        self.slot_scores[used] = by_id[slots[used, 2]]
        self.max_probe, self.lmax = self.hash.max_probe, min(self.hash.lmax, MAX_WORD)

    def find(self, cps: Sequence[int], h: int) -> Optional[Tuple[int, float]]:
        """(id, score) or None, looking at no more than max_probe slots."""
        vh = self.hash
        mask, n = vh.n_slots - 1, len(cps)
        s = wp._home(h, mask)
        for p in range(vh.max_probe):
            q = (s + p) & mask
            off, ln, idx, hh = (int(x) & 0xFFFFFFFF for x in vh.slots[q])
            if ln == 0:
                return None
            if hh == h and ln == n and all(int(vh.pool[off + k]) == cps[k] for k in range(n)):
                return idx, float(self.slot_scores[q])
        return None


# ---- the kernel's algorithm in Python ----------------------------------------------------------------------------------------------
def table_words(text: str, table: UnigramTable, opts: int) -> Optional[List[List[int]]]:
    """The words of `text` (code points, each word opening with U+2581) from the table and the option bits alone; None for a
    text with a FALLBACK code point.  The kernel's steps 2 and 3, without the tiles."""
    raw: List[Tuple[int, int]] = []
    for i, ch in enumerate(text):
        cp = ord(ch)
        if table.crlf and cp == 0x0D and text[i + 1: i + 2] == "\n":
            continue
        cls, rep = table.lookup(cp)
        if cls == FALLBACK:
            return None
        raw.extend(rep)
    collapse, single_meta, run_meta = (bool(opts & b) for b in (nat.UNIGRAM_COLLAPSE, nat.UNIGRAM_SINGLE_META, nat.UNIGRAM_RUN_META))
    n = len(raw)
    is_sp = [k == K_SP for _, k in raw]

    def sp_is_meta(i: int) -> bool:
        run = collapse and ((i > 0 and is_sp[i - 1]) or (i + 1 < n and is_sp[i + 1]))
        return run_meta if run else single_meta

    fin: List[int] = []
    for i, (cp, kind) in enumerate(raw):
        if kind == K_BRK:
            continue
        if kind == K_META:
            fin.append(META_CP)
        elif kind == K_SP:
            if sp_is_meta(i) and not (collapse and i > 0 and is_sp[i - 1]):
                fin.append(META_CP)
        else:
            after_end = i == 0 or raw[i - 1][1] == K_BRK or (is_sp[i - 1] and not sp_is_meta(i - 1))
            if after_end:
                fin.append(META_CP)
            fin.append(cp)
    words: List[List[int]] = []
    for cp in fin:
        if cp == META_CP:
            words.append([cp])
        else:
            words[-1].append(cp)
    return words


def emulate_word(w: Sequence[int], vocab: UnigramVocab, unk_id: int, unk_score: float, add=lambda a, b: a + b) -> List[int]:
    """The kernel's step 4 on one word: running FNV-1a hash per start, strictly-greater replacement, unknown candidates, fused
    unknowns.  `add` sums two scores (the near-tie test passes an fp32 one)."""
    n = len(w)
    best, back, tok = [0.0] * n, [-1] * n, [0] * n          # slot e: the path that ends behind element e
    for s in range(n):
        till = best[s - 1] if s else 0.0
        single, h = False, wp._SEED_WORD
        for e in range(s, min(n, s + vocab.lmax)):
            h = ((h ^ w[e]) * wp._FNV_PRIME) & 0xFFFFFFFF
            hit = vocab.find(w[s: e + 1], h)
            if hit is None:
                continue
            cand = add(hit[1], till)
            if back[e] < 0 or cand > best[e]:
                best[e], back[e], tok[e] = cand, s, hit[0]
            if e == s:
                single = True
        if not single:
            cand = add(unk_score, till)
            if back[s] < 0 or cand > best[s]:
                best[s], back[s], tok[s] = cand, s, unk_id
    out: List[int] = []
    e = n
    while e > 0:
        if not (tok[e - 1] == unk_id and out and out[-1] == unk_id):
            out.append(tok[e - 1])
        e = back[e - 1]
    return out[::-1]


def emulate_encode(text: str, table: UnigramTable, vocab: UnigramVocab, spec: UnigramSpec, max_len: int,
                   add=lambda a, b: a + b) -> Optional[List[int]]:
    """<s> ids </s> as the kernel computes them, or None for a text it flags: a FALLBACK code point, or a word of more than
    MAX_WORD code points (its U+2581 included)."""
    words = table_words(text, table, spec.opts)
    if words is None or any(len(w) > MAX_WORD for w in words):
        return None
    ids: List[int] = []
    budget = max_len - 2
    for w in words:
        if len(ids) >= budget:
            break
        ids.extend(emulate_word(w, vocab, spec.unk_id, spec.unk_score, add))
    return [spec.cls_id] + ids[:budget] + [spec.sep_id]


# ---- device side -------------------------------------------------------------------------------------------------------------------
class UnigramDeviceTokenizer:
    """The tables of one Unigram tokeniser on one device, and the launch; the interface of rag._wordpiece.DeviceTokenizer."""

    def __init__(self, tok, device):
        import torch
        self.spec = spec = unigram_spec(tok)
        self.device = torch.device(device)
        self.table = table_for_spec(spec)
        self.vocab = UnigramVocab(spec.pipeline.vocab)
        to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(self.device)   # noqa: E731
        self.d_table, self.d_rep = to_dev(self.table.entries), to_dev(self.table.pool)
        self.d_slots, self.d_pool = to_dev(self.vocab.hash.slots), to_dev(self.vocab.hash.pool)
        self.d_scores = torch.from_numpy(self.vocab.slot_scores).to(self.device)
        self.opts = spec.opts | (nat.UNIGRAM_CRLF if self.table.crlf else 0)
        self.added_rx = re.compile("|".join(re.escape(a) for a in spec.added)) if spec.added else None

    def encode(self, texts: Sequence[str], max_len: int, timings: Optional[dict] = None):
        """-> (ids cuda int32 [n, max_len], lens cuda int32 [n], flags cuda int32 [n], host: indices the host must tokenise
        whatever the flags say).  One launch, no synchronisation."""
        import torch
        t0 = time.perf_counter()
        blob, offsets, host = wp.encode_utf8(texts, self.added_rx)
        t1 = time.perf_counter()
        d_blob = torch.frombuffer(bytearray(blob or b"\0"), dtype=torch.uint8).to(self.device, non_blocking=True)
        d_off = torch.from_numpy(offsets).to(self.device, non_blocking=True)
        if timings is not None:
            torch.cuda.synchronize(self.device)
            t2 = time.perf_counter()
        sp = self.spec
        ids, lens, flags = nat.unigram_encode(d_blob, d_off, len(blob), self.d_table, self.d_rep, self.d_slots, self.d_scores, self.d_pool,
                                              self.vocab.max_probe, self.vocab.lmax, sp.unk_score, self.opts, sp.unk_id, sp.cls_id,
                                              sp.sep_id, sp.pad_id, max_len)
        if timings is not None:
            torch.cuda.synchronize(self.device)
            t3 = time.perf_counter()
            timings["host_encode_s"] = timings.get("host_encode_s", 0.0) + (t1 - t0)
            timings["h2d_s"] = timings.get("h2d_s", 0.0) + (t2 - t1)
            timings["kernel_s"] = timings.get("kernel_s", 0.0) + (t3 - t2)
        return ids, lens, flags, host


def device_tokenizer(tok, device):
    """The device tokeniser of `tok`: csrc/unigram.hip for a Unigram tokeniser, csrc/wordpiece.hip for the others."""
    return UnigramDeviceTokenizer(tok, device) if is_unigram(tok) else wp.DeviceTokenizer(tok, device)
