"""Host-side BERT tokeniser (uncased basic tokenisation + greedy WordPiece).

The reference gets this from tokenizers==0.22.1 via sentence-transformers (rag/embedding.py:33,65;
requirements.txt:148); the algorithm restated here is the published BERT one: clean -> lower-case
+ accent strip -> whitespace / punctuation split -> longest-match-first WordPiece with '##'
continuations, words longer than 100 chars -> [UNK], then [CLS] ... [SEP] (or the special tokens the
model directory names: MPNet's <s> ... </s>) with truncation to the model's max_seq_length.  ``HashTokenizer`` stands in when no vocab.txt exists (synthetic weights):
same splitting, ids from a stable hash, so plumbing and benchmarks run fully offline.
"""
from __future__ import annotations

import os
import re
import unicodedata
import zlib
from typing import Dict, List, Sequence, Tuple

import numpy as np


def _is_punct(ch: str) -> bool:
    cp = ord(ch)
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:
        return True
    return unicodedata.category(ch).startswith("P")


def _is_cjk(cp: int) -> bool:
    return (0x4E00 <= cp <= 0x9FFF or 0x3400 <= cp <= 0x4DBF or 0x20000 <= cp <= 0x2A6DF or
            0x2A700 <= cp <= 0x2B73F or 0x2B740 <= cp <= 0x2B81F or 0x2B820 <= cp <= 0x2CEAF or
            0xF900 <= cp <= 0xFAFF or 0x2F800 <= cp <= 0x2FA1F)


_ASCII_CTRL = {c: None for c in list(range(0, 9)) + [11, 12] + list(range(14, 32)) + [127]}   # Cc except \t \n \r
_ASCII_TOKEN = re.compile(r"[0-9A-Za-z]+|[!-/:-@\[-`{-~]")


def basic_tokenize(text: str, lower: bool = True, strip_accents=None) -> List[str]:
    """BERT basic tokenisation.  `strip_accents=None` follows the lower-casing flag (the BertNormalizer rule)."""
    if text.isascii():
        # same result as the general path below for 7-bit text (no accents, no CJK, every printable non-alphanumeric
        # character is punctuation and stands alone), two orders of magnitude faster: the MMR step re-tokenises the
        # retrieved page-long chunks on every query (reference rag/retrieval.py:238-239)
        text = text.translate(_ASCII_CTRL)
        return _ASCII_TOKEN.findall(text.lower() if lower else text)
    strip = lower if strip_accents is None else bool(strip_accents)
    cleaned = []
    for ch in text:
        cp = ord(ch)
        if cp == 0 or cp == 0xFFFD or (unicodedata.category(ch) in ("Cc", "Cf") and ch not in "\t\n\r"):
            continue
        if _is_cjk(cp):
            cleaned.append(f" {ch} ")
        elif ch in " \t\n\r" or unicodedata.category(ch) == "Zs":
            cleaned.append(" ")
        else:
            cleaned.append(ch)
    words: List[str] = []
    for tok in "".join(cleaned).split():
        if lower:
            tok = tok.lower()
        if strip:
            tok = "".join(c for c in unicodedata.normalize("NFD", tok) if unicodedata.category(c) != "Mn")
        cur = ""
        for ch in tok:
            if _is_punct(ch):
                if cur:
                    words.append(cur)
                    cur = ""
                words.append(ch)
            else:
                cur += ch
        if cur:
            words.append(cur)
    return words


def pair_lengths(n_a: int, n_b: int, budget: int) -> Tuple[int, int]:
    """Tokens each side of a pair keeps under transformers' truncation='longest_first' when `budget` tokens may remain in all
    (max_seq minus the three special tokens), as the `tokenizers` backend of transformers computes it: nothing is cut when the
    pair fits; else the shorter side is kept whole and the longer one cut to the rest, unless the shorter side is itself longer
    than the other's share -- then both are cut to budget // 2, and when the budget is odd the extra token goes to the side that
    was LONGER.  Tie rule: sides of equal length give the extra token to the SECOND text.  (Dropping one
    token at a time from the longer side, as the pure-Python tokenizers of older transformers did, ends within one token of
    this; the closed form is what the installed library computes, and tests/test_crossenc_cpu.py pins it against that.)"""
    if n_a + n_b <= budget:
        return n_a, n_b
    swap = n_a > n_b
    n1, n2 = (n_b, n_a) if swap else (n_a, n_b)            # n1 <= n2
    n2 = n1 if n1 > budget else max(n1, budget - n1)
    if n1 + n2 > budget:
        n1 = budget // 2
        n2 = n1 + budget % 2
    return (n2, n1) if swap else (n1, n2)


def join_pair(a_ids: Sequence[int], b_ids: Sequence[int], cls_id: int, sep_id: int, max_seq: int,
              n_a: int = None, n_b: int = None, seps: int = 1, typed: bool = True) -> Tuple[List[int], List[int]]:
    """[CLS] a [SEP] b [SEP] with token types 0 0 .. 0 1 .. 1 from the two sides' ids WITHOUT special tokens, cut by
    pair_lengths to max_seq tokens in all.  n_a / n_b: the sides' full token counts when a_ids / b_ids are already cut (to no
    fewer than max_seq - 3 tokens) -- the rule looks at the full lengths.  `seps=2, typed=False` is XLM-RoBERTa's pair,
    <s> a </s></s> b </s> with every type id 0: four special tokens."""
    if max_seq < 5:
        raise ValueError("a pair needs max_seq >= 5: three special tokens and room for a token of each side")
    k_a, k_b = pair_lengths(len(a_ids) if n_a is None else n_a, len(b_ids) if n_b is None else n_b, max_seq - 2 - seps)
    a, b = list(a_ids[:k_a]), list(b_ids[:k_b])
    return ([cls_id] + a + [sep_id] * seps + b + [sep_id],
            [0] * (len(a) + 1 + seps) + [1 if typed else 0] * (len(b) + 1))


class _PairMixin:
    """encode_pair for any tokenizer with encode(text, max_len) -> [cls] ids [sep] and cls_id / sep_id."""
    pair_seps, pair_typed = 1, True           # join_pair's format: BERT's; the Unigram (XLM-RoBERTa) tokenisers say 2, False

    def encode_body(self, text: str) -> List[int]:
        """All token ids of `text`, no special tokens, no truncation."""
        return self.encode(text, 1 << 30)[1:-1]

    def encode_pair(self, a: str, b: str, max_seq: int) -> Tuple[List[int], List[int]]:
        """(ids, type_ids) of [CLS] a [SEP] b [SEP], truncated to max_seq by the 'longest_first' rule (pair_lengths)."""
        return join_pair(self.encode_body(a), self.encode_body(b), self.cls_id, self.sep_id, max_seq, seps=self.pair_seps,
                         typed=self.pair_typed)


class WordPieceTokenizer(_PairMixin):
    def __init__(self, vocab: Dict[str, int], lower: bool = True, unk="[UNK]", cls="[CLS]", sep="[SEP]", pad="[PAD]",
                 strip_accents=None):
        self.vocab, self.lower, self.strip_accents = vocab, lower, strip_accents
        self.unk_id, self.cls_id, self.sep_id = vocab[unk], vocab[cls], vocab[sep]
        self.pad_id = vocab.get(pad, 0)

    @classmethod
    def from_vocab_file(cls, path: str, lower: bool = True, strip_accents=None, special=None) -> "WordPieceTokenizer":
        with open(path, encoding="utf-8") as fh:
            vocab = {line.rstrip("\n"): i for i, line in enumerate(fh)}
        return cls(vocab, lower=lower, strip_accents=strip_accents, **(special or {}))

    def _wordpiece(self, word: str) -> List[int]:
        if len(word) > 100:
            return [self.unk_id]
        out, start = [], 0
        while start < len(word):
            end, found = len(word), None
            while start < end:
                piece = ("##" if start else "") + word[start:end]
                if piece in self.vocab:
                    found = self.vocab[piece]
                    break
                end -= 1
            if found is None:
                return [self.unk_id]
            out.append(found)
            start = end
        return out

    def encode(self, text: str, max_len: int) -> List[int]:
        ids: List[int] = []
        for w in basic_tokenize(text, self.lower, self.strip_accents):
            ids.extend(self._wordpiece(w))
            if len(ids) >= max_len - 2:
                break
        return [self.cls_id] + ids[: max_len - 2] + [self.sep_id]


class FastWordPieceTokenizer(_PairMixin):
    """The same tokenisation through the `tokenizers` library (the reference's own backend: requirements.txt:148,
    via sentence-transformers) when it is importable: BertNormalizer + BertPreTokenizer + WordPiece, or the model
    directory's tokenizer.json as shipped.  Two orders of magnitude faster than the restatement above, which
    matters on the index-build side (the encoder takes ~17 M tokens/s).  `WordPieceTokenizer` stays the fallback
    and the specification; tests/test_host_cpu.py holds the two to identical ids."""

    def __init__(self, tok, cls_id: int, sep_id: int, pad_id: int):
        self._tok, self.cls_id, self.sep_id, self.pad_id = tok, cls_id, sep_id, pad_id
        self._max_len = None

    @classmethod
    def from_tokenizer_json(cls, path: str, special=None) -> "FastWordPieceTokenizer":
        """The model directory's own tokenizer.json, exactly as the reference's backend loads it (normaliser,
        casing and accent rules included); padding off, truncation set per call.  `special` names the model's
        special tokens (special_tokens_from_model_dir; default: read from the directory of `path`)."""
        from tokenizers import Tokenizer
        tok = Tokenizer.from_file(path)
        tok.no_padding()
        sp = special or special_tokens_from_model_dir(os.path.dirname(path))
        ids = [tok.token_to_id(sp[t]) for t in ("cls", "sep", "pad")]
        if ids[0] is None or ids[1] is None:
            raise ValueError(f"{path}: not a WordPiece tokenizer of this family ({sp['cls']} / {sp['sep']} missing)")
        return cls(tok, ids[0], ids[1], ids[2] if ids[2] is not None else 0)

    @classmethod
    def from_vocab(cls, vocab: Dict[str, int], lower: bool = True, unk="[UNK]", cls_tok="[CLS]", sep="[SEP]", pad="[PAD]",
                   strip_accents=None):
        from tokenizers import Tokenizer
        from tokenizers.models import WordPiece
        from tokenizers.normalizers import BertNormalizer
        from tokenizers.pre_tokenizers import BertPreTokenizer
        from tokenizers.processors import TemplateProcessing
        tok = Tokenizer(WordPiece(vocab, unk_token=unk, max_input_chars_per_word=100))
        tok.normalizer = BertNormalizer(clean_text=True, handle_chinese_chars=True, strip_accents=strip_accents, lowercase=lower)
        tok.pre_tokenizer = BertPreTokenizer()
        tok.post_processor = TemplateProcessing(single=f"{cls_tok} $A {sep}",
                                                special_tokens=[(cls_tok, vocab[cls_tok]), (sep, vocab[sep])])
        return cls(tok, vocab[cls_tok], vocab[sep], vocab.get(pad, 0))

    @classmethod
    def from_vocab_file(cls, path: str, lower: bool = True, strip_accents=None, special=None) -> "FastWordPieceTokenizer":
        with open(path, encoding="utf-8") as fh:
            vocab = {line.rstrip("\n"): i for i, line in enumerate(fh)}
        sp = dict(special or {})
        if "cls" in sp:
            sp["cls_tok"] = sp.pop("cls")
        return cls.from_vocab(vocab, lower=lower, strip_accents=strip_accents, **sp)

    def _limit(self, max_len: int):
        if self._max_len != max_len:
            self._tok.enable_truncation(max_length=max_len)
            self._max_len = max_len

    def encode(self, text: str, max_len: int) -> List[int]:
        self._limit(max_len)
        return self._tok.encode(text).ids

    def encode_batch(self, texts: Sequence[str], max_len: int) -> List[List[int]]:
        self._limit(max_len)
        return [e.ids for e in self._tok.encode_batch(list(texts))]


class BpeTokenizer(FastWordPieceTokenizer):
    """A byte-level BPE tokenizer.json (ModernBERT checkpoints) through the `tokenizers` library, as shipped: normaliser,
    ByteLevel pre-tokeniser, merges and the post-processor that adds [CLS] ... [SEP]; truncation to max_len per call.  There is no
    restatement in this package and no device kernel: without the library it cannot be loaded."""

    @classmethod
    def from_tokenizer_json(cls, path: str, special=None) -> "BpeTokenizer":
        try:
            return super().from_tokenizer_json(path, special=special)
        except ImportError as e:
            raise ImportError(f"{path} is a byte-level BPE tokenizer.json: loading it needs the `tokenizers` library, which is not "
                              f"installed (this package restates WordPiece and Unigram only)") from e

    def encode_body(self, text: str) -> List[int]:
        self._tok.no_truncation()
        self._max_len = None
        return self._tok.encode(text, add_special_tokens=False).ids


def make_wordpiece_tokenizer(vocab_path: str, lower: bool = True, strip_accents=None, special=None):
    """FastWordPieceTokenizer when the `tokenizers` library is importable (CRS_TOKENIZER=python forces the pure
    Python restatement), else WordPieceTokenizer.  `special`: {"cls", "sep", "pad", "unk"} token strings (BERT's
    by default)."""
    if os.environ.get("CRS_TOKENIZER", "") != "python":
        try:
            return FastWordPieceTokenizer.from_vocab_file(vocab_path, lower=lower, strip_accents=strip_accents, special=special)
        except ImportError:
            pass
    return WordPieceTokenizer.from_vocab_file(vocab_path, lower=lower, strip_accents=strip_accents, special=special)


_BERT_SPECIAL = {"cls": "[CLS]", "sep": "[SEP]", "pad": "[PAD]", "unk": "[UNK]"}


def special_tokens_from_model_dir(path: str) -> Dict[str, str]:
    """{"cls", "sep", "pad", "unk"} -> token string, as the model directory names them: special_tokens_map.json
    (cls_token / sep_token / pad_token / unk_token, plain strings or {"content": ...}), then what tokenizer.json
    itself says (the post-processor's first and last special token, the WordPiece model's unk_token, the padding
    block), then BERT's names.  MPNet directories give <s> </s> <pad> <unk>."""
    import json
    out: Dict[str, str] = {}
    sm = os.path.join(path, "special_tokens_map.json")
    if os.path.exists(sm):
        with open(sm, encoding="utf-8") as fh:
            m = json.load(fh)
        for key in ("cls", "sep", "pad", "unk"):
            v = m.get(key + "_token")
            v = v.get("content") if isinstance(v, dict) else v
            if isinstance(v, str):
                out[key] = v
    tj = os.path.join(path, "tokenizer.json")
    if len(out) < 4 and os.path.exists(tj):
        with open(tj, encoding="utf-8") as fh:
            t = json.load(fh)
        post = t.get("post_processor") or {}
        if post.get("type") == "TemplateProcessing":
            sp = [p["SpecialToken"]["id"] for p in post.get("single", []) if "SpecialToken" in p]
            if len(sp) >= 2:
                out.setdefault("cls", sp[0])
                out.setdefault("sep", sp[-1])
        elif isinstance(post.get("cls"), list) and isinstance(post.get("sep"), list):     # BertProcessing / RobertaProcessing
            out.setdefault("cls", post["cls"][0])
            out.setdefault("sep", post["sep"][0])
        unk = (t.get("model") or {}).get("unk_token")
        if isinstance(unk, str):
            out.setdefault("unk", unk)
        pad = (t.get("padding") or {}).get("pad_token")
        if isinstance(pad, str):
            out.setdefault("pad", pad)
        elif "pad" not in out and out.get("cls", "[CLS]").startswith("<"):
            out["pad"] = "<pad>"
    return {**_BERT_SPECIAL, **out}


def tokenizer_from_model_dir(path: str):
    """The tokeniser a HuggingFace BERT, MPNet or XLM-RoBERTa checkpoint directory describes (WordPiece, or Unigram when
    tokenizer.json's model.type says so; the special tokens are the directory's own: special_tokens_from_model_dir).  Casing comes from the TOKENIZER's own
    files, as in the reference stack (sentence-transformers hands the text to the HF tokenizer; the published
    all-MiniLM-L6-v2 ships sentence_bert_config.json do_lower_case=false next to an uncased vocab whose tokenizer
    lower-cases): tokenizer.json when the `tokenizers` library can load it, else vocab.txt with
    tokenizer_config.json's do_lower_case / strip_accents (absent -> lower-case, the uncased default)."""
    import json
    tj = os.path.join(path, "tokenizer.json")
    special = special_tokens_from_model_dir(path)
    if os.path.exists(tj):
        with open(tj, encoding="utf-8") as fh:
            model_type = (json.load(fh).get("model") or {}).get("type")
        if model_type == "Unigram":      # XLM-RoBERTa's SentencePiece model
            return make_unigram_tokenizer(tj, special=special)
        if model_type == "BPE":          # ModernBERT's byte-level BPE: the library only
            return BpeTokenizer.from_tokenizer_json(tj, special=special)
    if os.path.exists(tj) and os.environ.get("CRS_TOKENIZER", "") != "python":
        try:
            return FastWordPieceTokenizer.from_tokenizer_json(tj, special=special)
        except ImportError:
            pass
    lower, strip = True, None
    tc = os.path.join(path, "tokenizer_config.json")
    if os.path.exists(tc):
        with open(tc) as fh:
            cfg = json.load(fh)
        lower = bool(cfg.get("do_lower_case", True))
        strip = cfg.get("strip_accents", None)
    return make_wordpiece_tokenizer(os.path.join(path, "vocab.txt"), lower=lower, strip_accents=strip, special=special)


class HashTokenizer(_PairMixin):
    """vocab-free stand-in: one id per basic token, crc32 into [1000, vocab)."""

    def __init__(self, vocab_size: int, special=None, pair_seps: int = 1, pair_typed: bool = True):
        """`special` = (cls, sep, pad) ids; default BERT's (101, 102, 0), or (1, 2, 0) in a toy vocabulary.  pair_seps /
        pair_typed: the pair format (join_pair); 2, False stands in for an XLM-RoBERTa tokeniser."""
        self.vocab_size, self.pair_seps, self.pair_typed = vocab_size, pair_seps, pair_typed
        self.cls_id, self.sep_id, self.pad_id = special or ((101, 102, 0) if vocab_size > 1000 else (1, 2, 0))
        self.lo = 1000 if vocab_size > 2000 else max(3, max(self.cls_id, self.sep_id, self.pad_id) + 1)

    def encode(self, text: str, max_len: int) -> List[int]:
        span = self.vocab_size - self.lo
        ids = [self.lo + zlib.crc32(w.encode("utf-8")) % span for w in basic_tokenize(text)][: max_len - 2]
        return [self.cls_id] + ids + [self.sep_id]


def pad_batch(seqs: Sequence[Sequence[int]], pad_id: int = 0, short_steps: Sequence[int] = ()) -> Tuple[np.ndarray, np.ndarray]:
    """Right-pad to the longest sequence of the batch -> (ids int32 [B, S], lens int32 [B]).
    `short_steps` (ascending, e.g. (16, 32, 64)): a batch whose longest sequence fits one of them is padded
    up to it -- the fused short-sequence encoder kernels exist for exactly those lengths; padding is masked
    by `lens`, so the embeddings do not change."""
    lens = np.array([len(s) for s in seqs], dtype=np.int32)
    width = int(lens.max())
    for step in short_steps:
        if width <= step:
            width = step
            break
    out = np.full((len(seqs), width), pad_id, dtype=np.int32)
    for r, s in enumerate(seqs):
        out[r, : len(s)] = s
    return out, lens


# ---- Unigram (SentencePiece) tokenisation: XLM-RoBERTa checkpoints -------------------------------------------------------------------
META = "▁"
# Rust's char::is_whitespace (the White_Space property), which WhitespaceSplit splits on; str.isspace() also takes U+001C-1F
RUST_WHITESPACE = frozenset([0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000]
                            + list(range(0x2000, 0x200B)))
UNK_PENALTY = 10.0             # the unknown candidate's score is min_score - 10 (kUnkPenalty)


def _unsupported(field: str, got) -> NotImplementedError:
    return NotImplementedError(f"this Unigram tokenizer.json is not restated: {field} = {got!r}")


class UnigramPipeline:
    """What a Unigram tokenizer.json says, field by field (unigram_pipeline)."""

    def __init__(self):
        self.steps: List[tuple] = []        # ("nfkc",) ("nfc",) ("lower",) ("strip", left, right) ("replace", pattern, content) ("precompiled", b64)
        self.ws_split = False               # WhitespaceSplit in front of Metaspace
        self.prepend = "always"             # Metaspace prepend_scheme
        self.vocab: List[Tuple[str, float]] = []
        self.unk_id = 0
        self.single: List[tuple] = []       # ("special", id) / ("seq", "A")
        self.pair: List[tuple] = []         # the same with type ids: ("special", id, type) / ("seq", "A" | "B", type)
        self.added: List[dict] = []


def unigram_pipeline(cfg: dict) -> UnigramPipeline:
    """The restated fields of a tokenizer.json with model.type Unigram; NotImplementedError, naming the field, for any other."""
    p = UnigramPipeline()
    norm = cfg.get("normalizer")
    norms = [] if norm is None else norm["normalizers"] if norm.get("type") == "Sequence" else [norm]
    for i, n in enumerate(norms):
        kind, where = n.get("type"), f"normalizer[{i}]"
        if kind == "NFKC":
            p.steps.append(("nfkc",))
        elif kind == "NFC":
            p.steps.append(("nfc",))
        elif kind == "Lowercase":
            p.steps.append(("lower",))
        elif kind == "Strip":
            p.steps.append(("strip", bool(n.get("strip_left", True)), bool(n.get("strip_right", True))))
        elif kind == "Precompiled":
            p.steps.append(("precompiled", n.get("precompiled_charsmap")))
        elif kind == "Replace":
            pat = n.get("pattern") or {}
            if pat != {"Regex": " {2,}"}:
                raise _unsupported(where + ".pattern", pat)
            if n.get("content") not in (META, " "):
                raise _unsupported(where + ".content", n.get("content"))
            p.steps.append(("replace", " {2,}", n["content"]))
        else:
            raise _unsupported(where + ".type", kind)
    pre = cfg.get("pre_tokenizer") or {}
    pres = pre.get("pretokenizers", []) if pre.get("type") == "Sequence" else [pre]
    if len(pres) == 2 and pres[0].get("type") == "WhitespaceSplit":
        p.ws_split, pres = True, pres[1:]
    if len(pres) != 1 or pres[0].get("type") != "Metaspace":
        raise _unsupported("pre_tokenizer.type", [x.get("type") for x in pres] if len(pres) != 1 else pres[0].get("type"))
    ms = pres[0]
    if ms.get("replacement", META) != META:
        raise _unsupported("pre_tokenizer.replacement", ms.get("replacement"))
    if "prepend_scheme" in ms:
        p.prepend = ms["prepend_scheme"]
    elif "add_prefix_space" in ms:                     # the spelling of tokenizers < 0.15
        p.prepend = "always" if ms["add_prefix_space"] else "never"
    if p.prepend not in ("always", "never", "first"):
        raise _unsupported("pre_tokenizer.prepend_scheme", p.prepend)
    if ms.get("split", True) is not True:
        raise _unsupported("pre_tokenizer.split", ms.get("split"))
    model = cfg.get("model") or {}
    if model.get("type") != "Unigram":
        raise _unsupported("model.type", model.get("type"))
    if model.get("byte_fallback", False):
        raise _unsupported("model.byte_fallback", model.get("byte_fallback"))
    if model.get("unk_id") is None:
        raise _unsupported("model.unk_id", None)
    p.vocab = [(str(t), float(sc)) for t, sc in model["vocab"]]
    p.unk_id = int(model["unk_id"])
    post = cfg.get("post_processor") or {}
    if post.get("type") != "TemplateProcessing":
        raise _unsupported("post_processor.type", post.get("type"))
    ids = {k: v["ids"] for k, v in (post.get("special_tokens") or {}).items()}
    for key, dst in (("single", p.single), ("pair", p.pair)):
        for part in post.get(key) or []:
            if "SpecialToken" in part:
                sp = part["SpecialToken"]
                if len(ids.get(sp["id"], ())) != 1:
                    raise _unsupported(f"post_processor.special_tokens[{sp['id']}].ids", ids.get(sp["id"]))
                dst.append(("special", int(ids[sp["id"]][0]), int(sp.get("type_id", 0))))
            else:
                dst.append(("seq", part["Sequence"]["id"], int(part["Sequence"].get("type_id", 0))))
    kinds = [x[0] for x in p.single]
    if kinds != ["special", "seq", "special"]:
        raise _unsupported("post_processor.single", post.get("single"))
    p.added = [a for a in cfg.get("added_tokens") or [] if a.get("content")]
    for a in p.added:
        if a.get("normalized") or a.get("single_word"):
            raise _unsupported(f"added_tokens[{a['content']}]", {k: a.get(k) for k in ("normalized", "single_word")})
    return p


def _library_normalizer(steps):
    """The `tokenizers` normaliser object of `steps` without their Replace entries (those look at neighbours)."""
    import base64
    from tokenizers import normalizers as N
    objs = []
    for st in steps:
        if st[0] == "nfkc":
            objs.append(N.NFKC())
        elif st[0] == "nfc":
            objs.append(N.NFC())
        elif st[0] == "lower":
            objs.append(N.Lowercase())
        elif st[0] == "strip":
            objs.append(N.Strip(left=st[1], right=st[2]))
        elif st[0] == "precompiled":
            objs.append(N.Precompiled(base64.b64decode(st[1])))
    return N.Sequence(objs)


def unigram_viterbi(word: str, pieces: Dict[str, Tuple[int, float]], lmax: int, unk_id: int, unk_score: float,
                    add=lambda a, b: a + b) -> List[int]:
    """The ids of one pre-token, as the library's Unigram::encode_optimized walks it: best[end] takes a candidate only when it is
    strictly greater, candidates come by start ascending (so among equal sums the earliest start wins); a start with no
    one-character piece gets an unknown candidate of one character at unk_score; unknown ids next to each other fuse into one.
    `add` sums two scores (fp64 by default: what the library does; the near-tie test passes an fp32 one)."""
    n = len(word)
    best: List[float] = [0.0] * (n + 1)
    back: List[int] = [-1] * (n + 1)
    tok: List[int] = [0] * (n + 1)
    for s in range(n):
        single = False
        for e in range(s + 1, min(n, s + lmax) + 1):
            hit = pieces.get(word[s:e])
            if hit is None:
                continue
            cand = add(best[s], hit[1])
            if back[e] < 0 or cand > best[e]:
                best[e], back[e], tok[e] = cand, s, hit[0]
            if e == s + 1:
                single = True
        if not single:
            cand = add(best[s], unk_score)
            if back[s + 1] < 0 or cand > best[s + 1]:
                best[s + 1], back[s + 1], tok[s + 1] = cand, s, unk_id
    out: List[int] = []
    e = n
    while e > 0:
        if not (tok[e] == unk_id and out and out[-1] == unk_id):
            out.append(tok[e])
        e = back[e]
    return out[::-1]


class UnigramTokenizer(_PairMixin):
    """The specification: a Unigram tokenizer.json in plain Python (normaliser, WhitespaceSplit + Metaspace, Viterbi over the
    fp64 scores, TemplateProcessing).  `Precompiled` (SentencePiece's charsmap) goes through the `tokenizers` library's own
    normaliser object and raises ImportError without it.  Added tokens are cut out of the raw text before normalisation (their
    lstrip / rstrip flags are not restated)."""
    pair_seps, pair_typed = 2, False

    def __init__(self, cfg: dict, special: Dict[str, str] = None):
        self.pipeline = p = unigram_pipeline(cfg)
        self.pieces: Dict[str, Tuple[int, float]] = {}
        for i, (t, sc) in enumerate(p.vocab):
            self.pieces[t] = (i, sc)              # a repeated piece keeps its last id, as the library's map does
        self.lmax = max((len(t) for t in self.pieces), default=1)
        self.unk_id = p.unk_id
        self.unk_score = min(sc for _, sc in p.vocab) - UNK_PENALTY
        self.cls_id, self.sep_id = p.single[0][1], p.single[2][1]
        sp = special or {}
        self.pad_id = self.pieces.get(sp.get("pad", "<pad>"), (0, 0.0))[0]
        if "cls" in sp and self.pieces.get(sp["cls"], (self.cls_id,))[0] != self.cls_id:
            raise ValueError(f"the post-processor opens with id {self.cls_id}, the model directory names {sp['cls']!r}")
        if p.pair:
            self.pair_seps = sum(1 for x in p.pair if x[0] == "special") - 2
            self.pair_typed = any(x[2] for x in p.pair)
        self._lib_norm = _library_normalizer(p.steps) if any(st[0] == "precompiled" for st in p.steps) else None
        self._added_rx = re.compile("(" + "|".join(re.escape(a["content"]) for a in p.added) + ")") if p.added else None

    @classmethod
    def from_tokenizer_json(cls, path: str, special=None) -> "UnigramTokenizer":
        import json
        with open(path, encoding="utf-8") as fh:
            return cls(json.load(fh), special or special_tokens_from_model_dir(os.path.dirname(path)))

    def normalize(self, text: str) -> str:
        steps = self.pipeline.steps
        if self._lib_norm is not None:            # every step but Replace in the library, then the Replace steps
            text = self._lib_norm.normalize_str(text)
            steps = [st for st in steps if st[0] == "replace"]
        for st in steps:
            if st[0] == "nfkc":
                text = unicodedata.normalize("NFKC", text)
            elif st[0] == "nfc":
                text = unicodedata.normalize("NFC", text)
            elif st[0] == "lower":
                text = text.lower()
            elif st[0] == "strip":
                ws = "".join(map(chr, sorted(RUST_WHITESPACE)))
                text = text.lstrip(ws) if st[1] else text
                text = text.rstrip(ws) if st[2] else text
            elif st[0] == "replace":
                text = re.sub(st[1], st[2], text)
        return text

    def pre_tokenize(self, text: str, first: bool = True) -> List[str]:
        """The pre-tokens of a normalised text: each opens with the metaspace (unless the prepend scheme leaves it off)."""
        p = self.pipeline
        if p.ws_split:
            words, cur = [], ""
            for ch in text:
                if ord(ch) in RUST_WHITESPACE:
                    if cur:
                        words.append(cur)
                    cur = ""
                else:
                    cur += ch
            if cur:
                words.append(cur)
        else:
            words = [text] if text else []
        out: List[str] = []
        for i, w in enumerate(words):
            w = w.replace(" ", META)
            if (p.prepend == "always" or (p.prepend == "first" and first and i == 0)) and not w.startswith(META):
                w = META + w
            cur = ""
            for ch in w:                          # split in front of every metaspace (MergedWithNext)
                if ch == META and cur:
                    out.append(cur)
                    cur = ""
                cur += ch
            if cur:
                out.append(cur)
        return out

    def _ids(self, text: str, limit: int) -> List[int]:
        ids: List[int] = []
        parts = self._added_rx.split(text) if self._added_rx is not None else [text]
        for k, part in enumerate(parts):
            if k & 1:                             # an added token, as written
                ids.append(self.pieces[part][0])
                continue
            for w in self.pre_tokenize(self.normalize(part), first=(k == 0)):
                ids.extend(unigram_viterbi(w, self.pieces, self.lmax, self.unk_id, self.unk_score))
                if len(ids) >= limit:
                    return ids[:limit]
        return ids[:limit]

    def encode_body(self, text: str) -> List[int]:
        return self._ids(text, 1 << 30)

    def encode(self, text: str, max_len: int) -> List[int]:
        return [self.cls_id] + self._ids(text, max_len - 2) + [self.sep_id]

    def encode_batch(self, texts: Sequence[str], max_len: int) -> List[List[int]]:
        return [self.encode(t, max_len) for t in texts]


class FastUnigramTokenizer(FastWordPieceTokenizer):
    """tokenizer.json as shipped, through the `tokenizers` library: what the product uses when the library is importable.
    `UnigramTokenizer` stays the specification and the fallback; tests/test_unigram_cpu.py holds the two to identical ids."""
    pair_seps, pair_typed = 2, False

    @classmethod
    def from_tokenizer_json(cls, path: str, special=None) -> "FastUnigramTokenizer":
        from tokenizers import Tokenizer
        tok = Tokenizer.from_file(path)
        tok.no_padding()
        sp = special or special_tokens_from_model_dir(os.path.dirname(path))
        ids = [tok.token_to_id(sp[t]) for t in ("cls", "sep", "pad")]
        if ids[0] is None or ids[1] is None:
            raise ValueError(f"{path}: {sp['cls']} / {sp['sep']} are not in the vocabulary")
        return cls(tok, ids[0], ids[1], ids[2] if ids[2] is not None else 0)

    def encode_body(self, text: str) -> List[int]:
        self._tok.no_truncation()
        self._max_len = None
        return self._tok.encode(text, add_special_tokens=False).ids


def make_unigram_tokenizer(tokenizer_json: str, special=None):
    """FastUnigramTokenizer when the `tokenizers` library is importable (CRS_TOKENIZER=python forces the restatement), else
    UnigramTokenizer."""
    if os.environ.get("CRS_TOKENIZER", "") != "python":
        try:
            return FastUnigramTokenizer.from_tokenizer_json(tokenizer_json, special=special)
        except ImportError:
            pass
    return UnigramTokenizer.from_tokenizer_json(tokenizer_json, special=special)
