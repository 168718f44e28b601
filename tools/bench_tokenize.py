#!/usr/bin/env python3
"""Timing of tokenisation in front of the encoder: the host tokeniser against the device kernel (csrc/wordpiece.hip), in one process.

Corpus: --texts seeded English-like texts of about --chars characters: Zipf draws from a generated vocabulary of 30 000 lower-case
words, some capitalised, commas and full stops, and --foreign per cent of the texts with accented words, CJK and Hangul runs.
The WordPiece vocabulary holds the 20 000 most frequent words, 4 000 '##' suffixes, every letter and digit with and without '##' and
the punctuation, so frequent words are one id and rare ones split.

(a) tokenise, WordPiece and the hash rule, max_seq 256, alternating host / device, --reps windows each after a warm-up, every
    window closed by a synchronise:
      host    EmbeddingModel.tokenize + pad_batch of every batch of 32 + the copy of each block to the device (what embed_device's
              host branch does before the encoder runs);
      device  EmbeddingModel.tokenize_device: UTF-8 encode, upload, the kernel, the read-back of lens / flags, host fallback rows.
    tokens/s counts the ids handed to the encoder (special tokens included).  One more device pass with a synchronise after every
    stage gives the split host encode / upload / kernel / read-back.
(b) embed_device of synthetic:minilm over the same texts under tokenize 'host' and 'device', alternating: texts/s.
--unigram runs the Unigram leg alone (csrc/unigram.hip): a SentencePiece-style vocabulary over the same corpus (`▁word` for the
20 000 most frequent words, suffixes, letters; scores -log of a Zipf rank), XLM-R's pipeline with NFKC, max_seq 256.  It reports
texts/s and tokens/s of the device path (UTF-8 encode, upload, kernel, read-back of lens / flags) and of the kernel alone, of the
`tokenizers` library's encode_batch on RAYON_NUM_THREADS threads (16 unless set), of the Python restatement on a sample, and the
share of texts the kernel flags for the host.
A JSON array, one record per line, to --out (and stdout)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "compressed-rag-suite_amd")):
    sys.path.insert(0, p)


def spread(ts):
    return {"median_s": round(statistics.median(ts), 5), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5), "reps": len(ts)}


def make_words(rng, n):
    import numpy as np
    letters = np.array(list("etaoinshrdlcumwfgypbvkjxqz"))
    p = 1.0 / np.arange(1, 27) ** 0.7
    p /= p.sum()
    words, seen = [], set()
    while len(words) < n:
        w = "".join(rng.choice(letters, size=int(rng.integers(2, 11)), p=p))
        if w not in seen:
            seen.add(w)
            words.append(w)
    return words


def make_corpus(n_texts, chars, foreign_pct, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    words = make_words(rng, 30_000)
    p = 1.0 / np.arange(1, len(words) + 1) ** 1.0
    cdf = np.cumsum(p / p.sum())
    foreign = ["café", "naïve", "Übung", "résumé", "中文分词", "한국어", "İstanbul", "straße"]
    texts = []
    for t in range(n_texts):
        ids = np.minimum(np.searchsorted(cdf, rng.random(chars // 5)), len(words) - 1)
        marks = rng.random(len(ids))
        with_foreign = rng.random() * 100 < foreign_pct
        parts, size = [], 0
        for i, m in zip(ids, marks):
            w = words[i]
            if m < 0.06:
                w = w.capitalize()
            if with_foreign and m > 0.9:
                w = foreign[int(m * 1e6) % len(foreign)]
            w += "," if 0.5 < m < 0.56 else "." if 0.56 <= m < 0.62 else ""
            parts.append(w)
            size += len(w) + 1
            if size >= chars:
                break
        texts.append(" ".join(parts))
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + words[:20_000]
    suffixes = sorted({w[k:] for w in words[20_000:] for k in (2, 3, 4) if len(w) > k})[:4_000]
    vocab += ["##" + s for s in suffixes]
    singles = list("abcdefghijklmnopqrstuvwxyz0123456789")
    vocab += singles + ["##" + c for c in singles] + list(".,!?-'") + ["中", "文", "分", "词", "cafe", "naive", "resume"]
    out, seen = [], set()
    for v in vocab:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return texts, {v: i for i, v in enumerate(out)}


def unigram_config(words):
    """A tokenizer.json (as a dict) over the corpus' words: XLM-R's pipeline with NFKC in place of the Precompiled charsmap."""
    import math
    meta = "\u2581"
    vocab = [("<s>", 0.0), ("<pad>", 0.0), ("</s>", 0.0), ("<unk>", 0.0), (meta, -3.0)]
    vocab += [(meta + w, -math.log(r + 2.0) - 2.0) for r, w in enumerate(words[:20_000])]
    suffixes = sorted({w[k:] for w in words[20_000:] for k in (2, 3, 4) if len(w) > k})[:4_000]
    vocab += [(x, -9.0 - 0.001 * i) for i, x in enumerate(suffixes)]
    vocab += [(meta + w[:k], -10.0 - 0.0001 * i) for i, w in enumerate(words[20_000:24_000]) for k in (2, 3)]
    singles = list("abcdefghijklmnopqrstuvwxyz0123456789.,!?-'") + ["\u4e2d", "\u6587", "\u5206", "\u8bcd", "\u00e9", "\u00ef", "\u00fc", "\u00df"]
    vocab += [(c, -12.0 - 0.01 * i) for i, c in enumerate(singles)] + [(c.upper(), -13.0 - 0.01 * i) for i, c in enumerate(singles[:26])]
    seen, out = set(), []
    for t, sc in vocab:
        if t not in seen:
            seen.add(t)
            out.append([t, sc])
    special = lambda t: {"SpecialToken": {"id": t, "type_id": 0}}      # noqa: E731
    seq = lambda t: {"Sequence": {"id": t, "type_id": 0}}              # noqa: E731
    return {"version": "1.0", "truncation": None, "padding": None,
            "added_tokens": [{"id": i, "content": t, "single_word": False, "lstrip": False, "rstrip": False, "normalized": False,
                              "special": True} for i, t in enumerate(("<s>", "<pad>", "</s>", "<unk>"))],
            "normalizer": {"type": "Sequence", "normalizers": [{"type": "NFKC"}, {"type": "Replace", "pattern": {"Regex": " {2,}"}, "content": meta}]},
            "pre_tokenizer": {"type": "Sequence", "pretokenizers": [{"type": "WhitespaceSplit"},
                                                                    {"type": "Metaspace", "replacement": meta, "prepend_scheme": "always", "split": True}]},
            "post_processor": {"type": "TemplateProcessing", "single": [special("<s>"), seq("A"), special("</s>")],
                               "pair": [special("<s>"), seq("A"), special("</s>"), special("</s>"), seq("B"), special("</s>")],
                               "special_tokens": {"<s>": {"id": "<s>", "ids": [0], "tokens": ["<s>"]}, "</s>": {"id": "</s>", "ids": [2], "tokens": ["</s>"]}}},
            "decoder": None, "model": {"type": "Unigram", "unk_id": 3, "vocab": out, "byte_fallback": False}}


def unigram_leg(args):
    """The Unigram records (see the module's docstring)."""
    os.environ.setdefault("RAYON_NUM_THREADS", "16")
    os.environ.setdefault("TOKENIZERS_PARALLELISM", "true")
    import numpy as np
    import torch
    from rag import _native as nat
    from rag import _unigram as ug
    from rag.tokenizer import FastUnigramTokenizer, UnigramTokenizer
    nat.require_gpu()
    rng = np.random.default_rng(0)
    words = make_words(rng, 30_000)                   # the first draw of make_corpus(seed=0): the corpus' own words
    texts, _ = make_corpus(args.texts, args.chars, args.foreign)
    texts = [t.strip() for t in texts]
    cfg = unigram_config(words)
    special = {"cls": "<s>", "sep": "</s>", "pad": "<pad>", "unk": "<unk>"}
    py_tok = UnigramTokenizer(cfg, special)
    lib_tok = None
    try:
        from tokenizers import Tokenizer
        lib = Tokenizer.from_str(json.dumps(cfg))
        lib.no_padding()
        lib_tok = FastUnigramTokenizer(lib, 0, 2, 1)
    except ImportError:
        pass
    max_seq = 256
    n_bytes = sum(len(t.encode("utf-8")) for t in texts)
    records = [{"what": "corpus", "texts": len(texts), "utf8_bytes": n_bytes, "vocab": len(cfg["model"]["vocab"]), "max_seq": max_seq}]
    t0 = time.perf_counter()
    dt = ug.device_tokenizer(lib_tok or py_tok, "cuda")
    built = time.perf_counter() - t0

    def device_pass(timings=None):
        ids, lens, flags, host = dt.encode(texts, max_seq, timings)
        back = torch.stack((lens, flags)).cpu().numpy()
        return ids, back

    ids, back = device_pass()
    n_tokens, flagged = int(back[0].sum()), int(back[1].sum())
    sample = list(range(0, len(texts), max(1, len(texts) // 256)))[:256]
    t0 = time.perf_counter()
    want = [py_tok.encode(texts[i], max_seq) for i in sample]
    py_s = time.perf_counter() - t0
    got = ids.cpu().numpy()
    wrong = sum(1 for i, w in zip(sample, want) if not back[1][i] and got[i, : back[0][i]].tolist() != w)
    dev_t, lib_t, kernel_t = [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        device_pass()
        dev_t.append(time.perf_counter() - t0)
        split = {}
        device_pass(split)
        kernel_t.append(split["kernel_s"])
        if lib_tok is not None:
            t0 = time.perf_counter()
            lib_ids = lib_tok.encode_batch(texts, max_seq)
            lib_t.append(time.perf_counter() - t0)
    rec = {"what": "unigram", "host_class": type(lib_tok or py_tok).__name__, "tokens": n_tokens, "flagged_texts": flagged,
           "flagged_share": round(flagged / len(texts), 4), "sample_rows_differing_from_restatement": wrong,
           "tables_s": round(built, 3), "device": spread(dev_t), "kernel": spread(kernel_t), "device_split_s": {k: round(v, 5) for k, v in split.items()},
           "device_texts_per_s": round(len(texts) / statistics.median(dev_t)), "device_tokens_per_s": round(n_tokens / statistics.median(dev_t)),
           "kernel_texts_per_s": round(len(texts) / statistics.median(kernel_t)), "kernel_tokens_per_s": round(n_tokens / statistics.median(kernel_t)),
           "python_texts_per_s": round(len(sample) / py_s, 1), "python_tokens_per_s": round(sum(len(w) for w in want) / py_s)}
    if lib_t:
        lib_tokens = sum(len(x) for x in lib_ids)
        rec.update({"library": spread(lib_t), "library_threads": int(os.environ["RAYON_NUM_THREADS"]),
                    "library_texts_per_s": round(len(texts) / statistics.median(lib_t)),
                    "library_tokens_per_s": round(lib_tokens / statistics.median(lib_t))})
    records.append(rec)
    print(json.dumps(rec), flush=True)
    return records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--texts", type=int, default=4096)
    ap.add_argument("--chars", type=int, default=2000)
    ap.add_argument("--foreign", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tokenize_bench.json"))
    ap.add_argument("--unigram", action="store_true", help="run the Unigram leg alone (default --out: profiles/tokenize_unigram_bench.json)")
    args = ap.parse_args()
    if args.unigram:
        out = args.out if args.out != ap.get_default("out") else os.path.join(ROOT, "profiles", "tokenize_unigram_bench.json")
        records = unigram_leg(args)
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as fh:
            fh.write("[\n" + ",\n".join(json.dumps(r) for r in records) + "\n]\n")
        return

    import numpy as np
    import torch
    from rag.embedding import EmbeddingModel
    from rag.tokenizer import FastWordPieceTokenizer, WordPieceTokenizer, pad_batch
    from rag import _wordpiece as wp

    texts, vocab = make_corpus(args.texts, args.chars, args.foreign)
    n_bytes = sum(len(t.encode("utf-8")) for t in texts)
    records = [{"what": "corpus", "texts": len(texts), "utf8_bytes": n_bytes, "vocab": len(vocab)}]
    model = EmbeddingModel({"model_name": "synthetic:minilm", "batch_size": 32})
    dev = model.model.device
    hash_tok = model.tokenizer
    try:
        piece_tok = FastWordPieceTokenizer.from_vocab(vocab)
    except ImportError:
        piece_tok = WordPieceTokenizer(vocab)

    def host_pass():
        seqs = model.tokenize(texts)
        pad = getattr(model.tokenizer, "pad_id", 0)
        total = 0
        for lo in range(0, len(seqs), 32):
            ids, lens = pad_batch(seqs[lo: lo + 32], pad, short_steps=(16, 32, 64))
            torch.from_numpy(ids).to(dev)
            torch.from_numpy(lens).to(dev)
            total += int(lens.sum())
        torch.cuda.synchronize()
        return total

    def device_pass(timings=None):
        ids, lens = model._tokenize_device(texts, timings)
        torch.cuda.synchronize()
        return int(lens.sum())

    for name, tok in (("wordpiece", piece_tok), ("hash", hash_tok)):
        model.tokenizer, model._device_tokenizer = tok, None
        t0 = time.perf_counter()
        n_dev = device_pass()                      # warm-up: builds the tables, loads the kernel
        first = time.perf_counter() - t0
        n_host = host_pass()
        assert n_dev == n_host, (n_dev, n_host)
        dt = model._device_tokenizer
        flagged = int(dt.encode([str(t).strip() for t in texts], model.shape.max_seq)[2].sum().item())
        host_t, dev_t = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            host_pass()
            host_t.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            device_pass()
            dev_t.append(time.perf_counter() - t0)
        split = {}
        device_pass(split)
        records.append({"what": "tokenize", "tokenizer": name, "host_class": type(tok).__name__, "tokens": n_host,
                        "fallback_texts": flagged, "first_device_call_s": round(first, 3),
                        "table_build_s": round(dt.table.build_seconds, 3), "host": spread(host_t), "device": spread(dev_t),
                        "host_tokens_per_s": round(n_host / statistics.median(host_t)),
                        "device_tokens_per_s": round(n_host / statistics.median(dev_t)),
                        "device_split_s": {k: round(v, 5) for k, v in split.items()}})
        print(json.dumps(records[-1]), flush=True)
    if isinstance(piece_tok, FastWordPieceTokenizer):
        records.append({"what": "library_disagreements", "seconds": round(wp.library_disagreements(piece_tok._tok, wp.norm_table(True, None))[1], 3),
                        "code_points": int(len(wp.library_disagreements(piece_tok._tok, wp.norm_table(True, None))[0]))})

    # (b) embed_device under both settings (hash rule: the synthetic model's own tokeniser)
    models = {mode: EmbeddingModel({"model_name": "synthetic:minilm", "batch_size": 256, "tokenize": mode}) for mode in ("host", "device")}
    times = {"host": [], "device": []}
    for mode in ("host", "device"):
        models[mode].embed_device(texts[:512])
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for mode in ("host", "device"):
            t0 = time.perf_counter()
            models[mode].embed_device(texts)
            torch.cuda.synchronize()
            times[mode].append(time.perf_counter() - t0)
    records.append({"what": "embed_device", "model": "synthetic:minilm", "batch_size": 256, "texts": len(texts),
                    **{mode: spread(ts) for mode, ts in times.items()},
                    **{mode + "_texts_per_s": round(len(texts) / statistics.median(ts)) for mode, ts in times.items()}})
    print(json.dumps(records[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(r) for r in records) + "\n]\n")


if __name__ == "__main__":
    main()
