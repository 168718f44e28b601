"""Test helper of the late-interaction tests: a ColBERT checkpoint directory written to disk, and the small corpus the GPU tests
index.  Plain numpy / json; nothing here touches a device."""
import os

import numpy as np

DIM = 32


def write_colbert_dir(path, *, linear=True, dim=DIM, markers=True, seed=0):
    """The sentence-encoder directory of tests/_modeldir.py (config.json, vocab.txt, tokenizer files, bert.* tensors) with a
    ColBERT head: ``linear.weight [dim, hidden]`` beside ``bert.*`` in model.safetensors (left out with linear=False).  With
    `markers` the last two vocabulary entries become [unused0] / [unused1] (the vocabulary keeps its size).  Returns the weights
    under the internal names."""
    from safetensors.numpy import load_file, save_file
    from _modeldir import write_model_dir
    weights, cfg = write_model_dir(path, seed=seed)
    if markers:
        vocab_path = os.path.join(path, "vocab.txt")
        vocab = open(vocab_path, encoding="utf-8").read().split("\n")[:-1]
        vocab[-2:] = ["[unused0]", "[unused1]"]
        with open(vocab_path, "w", encoding="utf-8") as fh:
            fh.write("\n".join(vocab) + "\n")
    disk = load_file(os.path.join(path, "model.safetensors"))
    if linear:
        rng = np.random.default_rng(seed + 7)
        weights["linear.weight"] = disk["linear.weight"] = (rng.standard_normal((dim, cfg["hidden_size"])) / 8.0).astype(np.float32)
    save_file(disk, os.path.join(path, "model.safetensors"))
    return weights


WORDS = ("retrieval augmented generation answers questions from compressed documents with a vector index and an encoder on the device "
         "while late interaction keeps one small vector per token of every chunk and scores a query token by token").split()
PUNCT = [",", ".", ";", "!", "?", "(", ")", "-"]


def corpus(n: int, seed: int = 0):
    """n chunk texts of 1 to 60 words with punctuation sprinkled in (single characters, which the index drops), one empty text and
    one far longer than doc_maxlen."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        k = int(rng.integers(1, 61))
        words = []
        for w in rng.choice(WORDS, k):
            words.append(str(w))
            if rng.random() < 0.2:
                words.append(str(rng.choice(PUNCT)))
        out.append(" ".join(words) + f" chunk{i}")
    if n > 3:
        out[1] = ""
        out[2] = " ".join(str(w) for w in rng.choice(WORDS, 400))
    return out


def queries(n: int, seed: int = 1):
    rng = np.random.default_rng(seed)
    return [" ".join(str(w) for w in rng.choice(WORDS, int(rng.integers(2, 12)))) + " ?" for _ in range(n)]
