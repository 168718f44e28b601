"""Host side of the device tokeniser (csrc/wordpiece.hip, `rag.embedding.tokenize: 'device'`).

Three things are built here, all from `rag.tokenizer`'s own rules, and handed to the kernel as flat arrays:

* ``norm_table(lower, strip_accents)``: `basic_tokenize` restated as ONE uint32 per code point -- a class (DROP, SPACE, ISOLATE,
  KEEP, FALLBACK) and the character's replacement after lower-casing / NFD / removal of `Mn` marks: 0 to 3 code points, each with
  an "is punctuation" bit.  A text that holds a FALLBACK code point is tokenised by the model's own host tokeniser instead.
* ``VocabHash``: the WordPiece vocabulary as an open-addressing hash table over a pool of code points; the `##` prefix is a bit.
* ``emulate_encode``: the kernel's algorithm in plain Python on those two structures (tests/test_wordpiece_cpu.py holds it to
  `WordPieceTokenizer.encode`; the kernel is held to the same ids on the GPU).

``DeviceTokenizer`` owns the device copies and launches ``crs_wordpiece_encode``.
"""
from __future__ import annotations

import functools
import json
import re
import time
import unicodedata
import zlib
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from rag.tokenizer import FastWordPieceTokenizer, HashTokenizer, WordPieceTokenizer, _is_cjk, _is_punct

DROP, SPACE, ISOLATE, KEEP, FALLBACK = 0, 1, 2, 3, 4
N_CODE_POINTS = 0x110000
MODE_WORDPIECE, MODE_HASH = 0, 1
MAX_WORD_CHARS = 100          # WordPiece's max_input_chars_per_word: a longer word is one [UNK]

# table entry: bits 0-2 class | bits 3-4 replacement length n | bits 5-7 punctuation bit of each replacement code point |
# bits 8-31: n == 1: the code point itself; n >= 2: offset of the n code points in the replacement pool; n == 0: 0
_CLS_MASK, _N_SHIFT, _P_SHIFT, _V_SHIFT = 7, 3, 5, 8

_FNV_PRIME = 16777619
_SEED_WORD = 2166136261
_SEED_CONT = 2166136261 ^ 0x9E3779B9


class NormTable:
    """entries uint32 [0x110000], pool uint32 [m] (m >= 1), lower / strip as resolved."""

    def __init__(self, entries: np.ndarray, pool: np.ndarray, lower: bool, strip: bool, build_seconds: float):
        self.entries, self.pool, self.lower, self.strip, self.build_seconds = entries, pool, lower, strip, build_seconds
        self._list = None            # entries as a Python list: lookup() is the emulation's inner loop

    def lookup(self, cp: int) -> Tuple[int, List[int], List[bool]]:
        """(class, replacement code points, their punctuation bits)"""
        if self._list is None:
            self._list = self.entries.tolist()
        e = self._list[cp]
        n = (e >> _N_SHIFT) & 3
        v = e >> _V_SHIFT
        rep = [] if n == 0 else [v] if n == 1 else [int(x) for x in self.pool[v: v + n]]
        return e & _CLS_MASK, rep, [bool((e >> (_P_SHIFT + i)) & 1) for i in range(n)]

    def fallback_mask(self) -> np.ndarray:
        return (self.entries & _CLS_MASK) == FALLBACK

    def with_fallback(self, code_points) -> "NormTable":
        """A copy whose listed code points are FALLBACK too."""
        ent = self.entries.copy()
        ent[np.asarray(list(code_points), dtype=np.int64)] = FALLBACK
        return NormTable(ent, self.pool, self.lower, self.strip, self.build_seconds)


@functools.lru_cache(maxsize=None)
def _norm_table(lower: bool, strip: bool) -> NormTable:
    t0 = time.perf_counter()
    ent = np.zeros(N_CODE_POINTS, dtype=np.uint32)
    pool: List[int] = [0]                      # offset 0 is never a valid replacement: entries with n >= 2 point past it
    cat, nfd, comb = unicodedata.category, unicodedata.normalize, unicodedata.combining
    for cp in range(N_CODE_POINTS):
        ch = chr(cp)
        c = cat(ch)
        if c in ("Co", "Cn", "Cs") or cp == 0x3A3:       # unassigned / private / surrogate: the host tokenisers drift there;
            ent[cp] = FALLBACK                           # U+03A3: str.lower() looks at the context (final sigma)
            continue
        if cp == 0 or cp == 0xFFFD or (c in ("Cc", "Cf") and ch not in "\t\n\r"):
            ent[cp] = DROP
            continue
        if ch in " \t\n\r" or c == "Zs" or cp in (0x2028, 0x2029):   # U+2028/9: not Zs, but str.split() splits on them
            ent[cp] = SPACE
            continue
        cls = ISOLATE if _is_cjk(cp) else KEEP
        rep = ch.lower() if lower else ch
        if strip:
            rep = "".join(x for x in nfd("NFD", rep) if cat(x) != "Mn")
            if any(comb(x) for x in rep):      # a non-Mn mark with a combining class: NFD of a whole word may reorder it
                ent[cp] = FALLBACK
                continue
        n = len(rep)
        if n > 3 or (cls == ISOLATE and n != 1):
            ent[cp] = FALLBACK
            continue
        if n == 0:
            ent[cp] = cls if cls == KEEP else SPACE
            continue
        bits = cls | (n << _N_SHIFT)
        for i, x in enumerate(rep):
            if _is_punct(x):
                bits |= 1 << (_P_SHIFT + i)
        if n == 1:
            ent[cp] = bits | (ord(rep) << _V_SHIFT)
        else:
            ent[cp] = bits | (len(pool) << _V_SHIFT)
            pool.extend(ord(x) for x in rep)
    return NormTable(ent, np.asarray(pool, dtype=np.uint32), lower, strip, time.perf_counter() - t0)


def norm_table(lower: bool = True, strip_accents=None) -> NormTable:
    """The per-code-point restatement of basic_tokenize(text, lower, strip_accents); built once per process and flag pair
    (about two seconds of `unicodedata` calls), and only when the device path asks for it."""
    strip = bool(lower) if strip_accents is None else bool(strip_accents)
    return _norm_table(bool(lower), strip)


# ---- words from the table (the specification of the kernel's first half) -----------------------------------------------------------
def table_words(text: str, table: NormTable) -> Optional[List[List[int]]]:
    """The words of `text` as lists of code points, using nothing but the table; None when the text holds a FALLBACK code point."""
    words: List[List[int]] = []
    cur: List[int] = []
    for ch in text:
        cls, rep, punct = table.lookup(ord(ch))
        if cls == FALLBACK:
            return None
        if cls == SPACE:
            if cur:
                words.append(cur)
                cur = []
            continue
        for x, p in zip(rep, punct):
            if p or cls == ISOLATE:
                if cur:
                    words.append(cur)
                    cur = []
                words.append([x])
            else:
                cur.append(x)
    if cur:
        words.append(cur)
    return words


# ---- vocabulary hash table ---------------------------------------------------------------------------------------------------------
def piece_hash(cps: Sequence[int], cont: bool) -> int:
    h = _SEED_CONT if cont else _SEED_WORD
    for c in cps:
        h = ((h ^ c) * _FNV_PRIME) & 0xFFFFFFFF
    return h


def _home(h: int, mask: int) -> int:
    return (h ^ (h >> 15)) & mask


class VocabHash:
    """Open addressing, linear probing, a power-of-two slot count >= 2 x entries.  slots int32 [n_slots, 4] =
    {offset into pool, length | continuation << 31, id, hash}; length 0 = empty.  pool uint32: the pieces' code points without
    the '##'.  max_probe: slots a lookup may have to look at; lmax: the longest piece (code points)."""

    def __init__(self, vocab: Dict[str, int], prefix: str = "##"):
        items = []
        for tok, idx in vocab.items():
            cont = bool(prefix) and tok.startswith(prefix) and len(tok) > len(prefix)     # prefix None: no continuation pieces (Unigram)
            body = tok[len(prefix):] if cont else tok
            if body:
                items.append((tuple(ord(c) for c in body), cont, int(idx)))
        n_slots = 4
        while n_slots < 2 * max(1, len(items)):
            n_slots *= 2
        mask = n_slots - 1
        slots = np.zeros((n_slots, 4), dtype=np.int64)
        pool: List[int] = []
        seen = {}
        max_probe, lmax = 1, 1
        for cps, cont, idx in items:
            if (cps, cont) in seen:        # a duplicated line of vocab.txt: the dict keeps the last id, and so does this table
                slots[seen[(cps, cont)], 2] = idx
                continue
            h = piece_hash(cps, cont)
            s, probes = _home(h, mask), 1
            while slots[s, 1] != 0:
                s, probes = (s + 1) & mask, probes + 1
            slots[s] = (len(pool), len(cps) | (int(cont) << 31), idx, h)
            seen[(cps, cont)] = s
            pool.extend(cps)
            max_probe, lmax = max(max_probe, probes), max(lmax, len(cps))
        self.n_slots, self.max_probe, self.lmax, self.n_entries = n_slots, max_probe, lmax, len(seen)
        self.slots = (slots & 0xFFFFFFFF).astype(np.uint32).view(np.int32).reshape(n_slots, 4)
        self.pool = np.asarray(pool or [0], dtype=np.uint32)

    def lookup(self, cps: Sequence[int], cont: bool, h: Optional[int] = None, count: Optional[list] = None) -> int:
        """id or -1; looks at no more than max_probe slots (`count`, a one-element list, receives the number looked at)."""
        h = piece_hash(cps, cont) if h is None else h
        mask, n = self.n_slots - 1, len(cps)
        tag = n | (int(cont) << 31)
        s = _home(h, mask)
        for p in range(self.max_probe):
            off, ln, idx, hh = (int(x) & 0xFFFFFFFF for x in self.slots[(s + p) & mask])
            if count is not None:
                count[0] = p + 1
            if ln == 0:
                return -1
            if hh == h and ln == tag and all(int(self.pool[off + k]) == cps[k] for k in range(n)):
                return idx if idx < (1 << 31) else idx - (1 << 32)
        return -1


# ---- the kernel's algorithm in Python ----------------------------------------------------------------------------------------------
def _utf8(cp: int) -> bytes:
    return chr(cp).encode("utf-8", "surrogatepass")


def emulate_encode(text: str, table: NormTable, max_len: int, *, vocab: Optional[VocabHash] = None, unk_id: int = 0, cls_id: int = 0,
                   sep_id: int = 0, hash_lo: int = 0, hash_span: int = 0) -> Optional[List[int]]:
    """[cls] ids [sep] as the kernel computes them (vocab given: WordPiece, longest match by growing the piece one code point at a
    time with a running hash; else the HashTokenizer rule), or None for a text with a FALLBACK code point."""
    words = table_words(text, table)
    if words is None:
        return None
    ids: List[int] = []
    budget = max_len - 2
    for w in words:
        if len(ids) >= budget:
            break
        if vocab is None:
            crc = 0
            for cp in w:
                crc = zlib.crc32(_utf8(cp), crc)
            ids.append(hash_lo + crc % hash_span)
            continue
        if len(w) > MAX_WORD_CHARS:
            ids.append(unk_id)
            continue
        out, start = [], 0
        while start < len(w):
            h = _SEED_CONT if start else _SEED_WORD
            best, best_end = -1, start
            for e in range(start, min(len(w), start + vocab.lmax)):
                h = ((h ^ w[e]) * _FNV_PRIME) & 0xFFFFFFFF
                idx = vocab.lookup(w[start: e + 1], start > 0, h)
                if idx >= 0:
                    best, best_end = idx, e + 1
            if best < 0:
                out = [unk_id]
                break
            out.append(best)
            start = best_end
        ids.extend(out)
    return [cls_id] + ids[:budget] + [sep_id]


# ---- what a tokeniser object asks of the kernel ------------------------------------------------------------------------------------
class TokenizerSpec:
    def __init__(self, mode, lower, strip_accents, vocab=None, unk_id=0, cls_id=0, sep_id=0, pad_id=0, hash_lo=0, hash_span=1,
                 library=None, added=()):
        self.mode, self.lower, self.strip_accents, self.vocab = mode, lower, strip_accents, vocab
        self.unk_id, self.cls_id, self.sep_id, self.pad_id, self.hash_lo, self.hash_span = unk_id, cls_id, sep_id, pad_id, hash_lo, hash_span
        self.library = library       # the `tokenizers` Tokenizer when the host tokeniser is that library's, else None
        self.added = tuple(added)    # its added tokens: matched in the raw text by the library, so such a text goes to the host


def _require(cond: bool, field: str, got) -> None:
    if not cond:
        raise NotImplementedError(f"tokenize: 'device' does not restate this tokenizer: {field} = {got!r}")


def tokenizer_spec(tok) -> TokenizerSpec:
    """What `tok` (HashTokenizer, WordPieceTokenizer or FastWordPieceTokenizer) computes, as the kernel's arguments; raises
    NotImplementedError, naming the field, for a tokenizer.json setting the device path does not restate."""
    if isinstance(tok, HashTokenizer):
        return TokenizerSpec(MODE_HASH, True, None, cls_id=tok.cls_id, sep_id=tok.sep_id, pad_id=tok.pad_id, hash_lo=tok.lo,
                             hash_span=tok.vocab_size - tok.lo)
    if isinstance(tok, WordPieceTokenizer):
        return TokenizerSpec(MODE_WORDPIECE, bool(tok.lower), tok.strip_accents, vocab=tok.vocab, unk_id=tok.unk_id, cls_id=tok.cls_id,
                             sep_id=tok.sep_id, pad_id=tok.pad_id)
    if isinstance(tok, FastWordPieceTokenizer):
        cfg = json.loads(tok._tok.to_str())
        norm, pre, model = cfg.get("normalizer") or {}, cfg.get("pre_tokenizer") or {}, cfg.get("model") or {}
        _require(norm.get("type") == "BertNormalizer", "normalizer.type", norm.get("type"))
        _require(norm.get("clean_text") is True, "normalizer.clean_text", norm.get("clean_text"))
        _require(norm.get("handle_chinese_chars") is True, "normalizer.handle_chinese_chars", norm.get("handle_chinese_chars"))
        _require(pre.get("type") == "BertPreTokenizer", "pre_tokenizer.type", pre.get("type"))
        _require(model.get("type") == "WordPiece", "model.type", model.get("type"))
        _require(model.get("continuing_subword_prefix") == "##", "model.continuing_subword_prefix", model.get("continuing_subword_prefix"))
        _require(model.get("max_input_chars_per_word") == MAX_WORD_CHARS, "model.max_input_chars_per_word", model.get("max_input_chars_per_word"))
        vocab = model["vocab"]
        _require(model.get("unk_token") in vocab, "model.unk_token", model.get("unk_token"))
        added = [a["content"] for a in cfg.get("added_tokens") or [] if a.get("content")]
        return TokenizerSpec(MODE_WORDPIECE, bool(norm.get("lowercase")), norm.get("strip_accents"), vocab=vocab,
                             unk_id=vocab[model["unk_token"]], cls_id=tok.cls_id, sep_id=tok.sep_id, pad_id=tok.pad_id,
                             library=tok._tok, added=added)
    raise NotImplementedError(f"tokenize: 'device' does not restate this tokenizer: {type(tok).__name__}")


# ---- where the `tokenizers` library and basic_tokenize part ways -------------------------------------------------------------------
_CONTEXTS = (("ab", "cd", False), ("", "", False), ("a", "", False), ("", "b", False), ("a", "b", True))


def _expected_words(table: NormTable, cp: int) -> List[str]:
    """The words of the five context strings around chr(cp), per the table, flattened."""
    cls, rep, punct = table.lookup(cp)
    out: List[str] = []
    for left, right, spaced in _CONTEXTS:
        if spaced:
            out.append(left)
            left_, right_ = "", ""
        else:
            left_, right_ = left, right
        if cls == SPACE:
            out.extend(x for x in (left_, right_) if x)
        else:
            cur = left_
            for x, p in zip(rep, punct):
                if p or cls == ISOLATE:
                    if cur:
                        out.append(cur)
                        cur = ""
                    out.append(chr(x))
                else:
                    cur += chr(x)
            cur += right_
            if cur:
                out.append(cur)
        if spaced:
            out.append(right)
    return out


def _context_lines(cp: int) -> str:
    ch = chr(cp)
    return "\n".join((l + " " + ch + " " + r) if sp else (l + ch + r) for l, r, sp in _CONTEXTS)


_library_cache: Dict[tuple, Tuple[np.ndarray, float]] = {}


def library_disagreements(library, table: NormTable) -> Tuple[np.ndarray, float]:
    """Code points outside the table's FALLBACK set on which the `tokenizers` normaliser + pre-tokeniser of `library` split or map
    the five context strings differently from the table (Unicode-version drift between the library and this Python) -> (sorted
    int64 array, seconds it took).  Bulk: eight thousand code points per library call.
    Cached per process and normaliser setting."""
    key = (json.dumps(json.loads(library.to_str()).get("normalizer"), sort_keys=True), table.lower, table.strip)
    if key in _library_cache:
        return _library_cache[key]
    t0 = time.perf_counter()
    normalizer, pre = library.normalizer, library.pre_tokenizer
    cps = np.nonzero(~table.fallback_mask())[0]
    cps = cps[cps != 0]                         # NUL: dropped by both; kept out of the probe strings
    entries = table.entries.tolist()
    fence = "zzzz"                              # a line of its own between two code points' lines: splits the library's word list

    def differing(block) -> List[int]:
        sep = "\n" + fence + "\n"
        text = sep.join([f"ab{ch}cd\n{ch}\na{ch}\n{ch}b\na {ch} b" for ch in map(chr, block.tolist())])
        words = [w for w, _ in pre.pre_tokenize_str(normalizer.normalize_str(text))]
        groups, cur = [], []
        for w in words:
            if w == fence:
                groups.append(cur)
                cur = []
            else:
                cur.append(w)
        groups.append(cur)
        if len(groups) != len(block):           # a code point swallowed a fence: halve until it stands alone
            if len(block) == 1:
                return [int(block[0])]
            half = len(block) // 2
            return differing(block[:half]) + differing(block[half:])
        out = []
        for c, g in zip(block.tolist(), groups):
            e = entries[c]
            if (e >> _N_SHIFT) & 3 == 1:        # one code point for one: nearly every entry; the general rule, unrolled
                x = chr(e >> _V_SHIFT)
                alone = (e >> _P_SHIFT) & 1 or e & _CLS_MASK == ISOLATE
                want = ["ab", x, "cd", x, "a", x, x, "b", "a", x, "b"] if alone else ["ab" + x + "cd", x, "a" + x, x + "b", "a", x, "b"]
            else:
                want = _expected_words(table, c)
            if g != want:
                out.append(c)
        return out

    bad: List[int] = []
    for i in range(0, len(cps), 8192):
        bad.extend(differing(cps[i: i + 8192]))
    res = (np.asarray(sorted(bad), dtype=np.int64), time.perf_counter() - t0)
    _library_cache[key] = res
    return res


def table_for_spec(spec: TokenizerSpec) -> NormTable:
    """The table the kernel gets for `spec`: norm_table of its flags, plus the library's disagreements when the host tokeniser
    is the `tokenizers` library one."""
    table = norm_table(spec.lower, spec.strip_accents)
    if spec.library is not None:
        extra, _ = library_disagreements(spec.library, table)
        if len(extra):
            table = table.with_fallback(extra)
    return table


# ---- device side -------------------------------------------------------------------------------------------------------------------
def encode_utf8(texts: Sequence[str], added_rx=None) -> Tuple[bytes, np.ndarray, List[int]]:
    """(blob, offsets int64 [n + 1], indices of texts that must go to the host tokeniser: a lone surrogate cannot be encoded, and
    the library matches its added tokens in the raw text)"""
    parts, host = [], []
    for i, t in enumerate(texts):
        try:
            b = t.encode("utf-8")
            if added_rx is not None and added_rx.search(t):
                raise ValueError
        except ValueError:                     # UnicodeEncodeError is one
            b = b""
            host.append(i)
        parts.append(b)
    offsets = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in parts], out=offsets[1:])
    return b"".join(parts), offsets, host


class DeviceTokenizer:
    """The tables of one tokeniser on one device, and the launch."""

    def __init__(self, tok, device):
        import torch
        self.spec = spec = tokenizer_spec(tok)
        self.device = torch.device(device)
        self.table = table_for_spec(spec)
        to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(self.device)   # noqa: E731
        self.d_table, self.d_rep = to_dev(self.table.entries), to_dev(self.table.pool)
        if spec.mode == MODE_WORDPIECE:
            self.vocab = VocabHash(spec.vocab)
            self.d_slots, self.d_pool = to_dev(self.vocab.slots), to_dev(self.vocab.pool)
            self.max_probe, self.lmax = self.vocab.max_probe, self.vocab.lmax
        else:
            self.vocab = None
            self.d_slots = torch.zeros((4, 4), dtype=torch.int32, device=self.device)
            self.d_pool = torch.zeros(1, dtype=torch.int32, device=self.device)
            self.max_probe, self.lmax = 1, 1
        self.added_rx = re.compile("|".join(re.escape(a) for a in spec.added), re.IGNORECASE) if spec.added else None

    def encode(self, texts: Sequence[str], max_len: int, timings: Optional[dict] = None):
        """-> (ids cuda int32 [n, max_len], lens cuda int32 [n], flags cuda int32 [n], host: indices the host must tokenise
        whatever the flags say).  One launch, no synchronisation."""
        import torch
        from rag import _native as nat
        t0 = time.perf_counter()
        blob, offsets, host = encode_utf8(texts, self.added_rx)
        t1 = time.perf_counter()
        d_blob = torch.frombuffer(bytearray(blob or b"\0"), dtype=torch.uint8).to(self.device, non_blocking=True)
        d_off = torch.from_numpy(offsets).to(self.device, non_blocking=True)
        if timings is not None:
            torch.cuda.synchronize(self.device)
            t2 = time.perf_counter()
        sp = self.spec
        ids, lens, flags = nat.wordpiece_encode(d_blob, d_off, len(blob), self.d_table, self.d_rep, self.d_slots, self.d_pool,
                                                self.max_probe, self.lmax, sp.mode, sp.unk_id, sp.cls_id, sp.sep_id, sp.pad_id,
                                                sp.hash_lo, sp.hash_span, max_len)
        if timings is not None:
            torch.cuda.synchronize(self.device)
            t3 = time.perf_counter()
            timings["host_encode_s"] = timings.get("host_encode_s", 0.0) + (t1 - t0)
            timings["h2d_s"] = timings.get("h2d_s", 0.0) + (t2 - t1)
            timings["kernel_s"] = timings.get("kernel_s", 0.0) + (t3 - t2)
        return ids, lens, flags, host
