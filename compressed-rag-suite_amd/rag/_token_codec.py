"""The codec of a 2-bit residual token index (``late_interaction: {token_dtype: 'res2'}``): unit fp16 centroids, three
residual cutoffs and four bucket weights, trained once per (store, encoder) on a seeded sample of the documents.

Training is host code over the project's own ops: the sample is encoded to fp16 by the encoder, spherical k-means assigns with the
nearest-centroid stage of crs_token_compress (csrc/token_compress.hip) and updates with index_add_, and the cutoffs / weights are
quantiles of the sample's residual coordinates.  Nothing here is a retrieval-quality claim: the format is the one ColBERTv2 ships,
the scores are an exactly specified function of the stored fields (csrc/maxsim_rc.h)."""
from __future__ import annotations

import math

import numpy as np

from . import _native as nat

KEYS = ("centroids", "train_docs", "kmeans_iters", "codec_seed")
TOKENS_PER_CENTROID = 32      # the training sample holds at least this many tokens per centroid
QUANTILE_SAMPLE = 1 << 22     # residual coordinates the quantiles are taken over (a seeded subset when there are more)


def parse_config(config: dict) -> dict:
    """The codec keys of a late_interaction dict with their types checked; unset keys get their defaults (centroids: None,
    resolved from the token count at build time)."""
    out = {}
    for key, default, low in (("centroids", None, nat.RC_MIN_CENTROIDS), ("train_docs", 4096, 1), ("kmeans_iters", 8, 1), ("codec_seed", 0, 0)):
        val = config.get(key, default)
        if val is not None and (not isinstance(val, (int, np.integer)) or isinstance(val, bool) or val < low):
            raise ValueError(f"late_interaction {key} must be an integer >= {low}, got {val!r}")
        out[key] = None if val is None else int(val)
    k = out["centroids"]
    if k is not None and (k > nat.RC_MAX_CENTROIDS or k & (k - 1)):
        raise ValueError(f"late_interaction centroids must be a power of two in {nat.RC_MIN_CENTROIDS}..{nat.RC_MAX_CENTROIDS}, got {k}")
    return out


def resolve_centroids(cfg: dict, tokens_expected: int, sample_tokens: int) -> int:
    """cfg's centroids, else the power of two nearest 16 sqrt(tokens expected), capped so that the training sample holds at least
    TOKENS_PER_CENTROID tokens per centroid; never below RC_MIN_CENTROIDS."""
    if cfg["centroids"] is not None:
        return cfg["centroids"]
    want = 16.0 * math.sqrt(max(tokens_expected, 1))
    lo = 1 << int(math.floor(math.log2(want)))
    k = lo if want - lo <= 2 * lo - want else 2 * lo
    while k > nat.RC_MIN_CENTROIDS and k * TOKENS_PER_CENTROID > sample_tokens:
        k //= 2
    return max(nat.RC_MIN_CENTROIDS, min(k, nat.RC_MAX_CENTROIDS))


def sample_rows(cfg: dict, n_docs: int) -> np.ndarray:
    """The documents of the training sample: train_docs of them, seeded, in ascending order."""
    rng = np.random.default_rng(cfg["codec_seed"])
    return np.sort(rng.permutation(n_docs)[: cfg["train_docs"]])


def index_bytes(tokens: int, dimp: int, centroids: int) -> int:
    """What max_index_bytes counts: the three planes and the centroid table."""
    return tokens * (dimp // 4 + 6) + centroids * dimp * 2


class TokenCodec:
    """centroids fp16 [K, dimp] (unit rows, zeros past dim), cutoffs fp32 [3], weights fp32 [4], on the index's device."""

    def __init__(self, centroids, cutoffs, weights, dim: int):
        self.centroids, self.cutoffs, self.weights, self.dim = centroids, cutoffs, weights, int(dim)

    @property
    def n_centroids(self) -> int:
        return int(self.centroids.shape[0])


def train(sample16, dim: int, n_centroids: int, cfg: dict) -> TokenCodec:
    """sample16 cuda fp16 [S, dimp] unit rows -> the codec.  The first centroids are seeded sample rows (cycled when the sample is
    smaller than the table); a cluster that loses every token keeps its centroid, so a run is a function of the sample and seed."""
    import torch
    dev, s = sample16.device, sample16.shape[0]
    if s == 0:
        raise ValueError("the codec's training sample holds no tokens")
    gen = torch.Generator(device="cpu").manual_seed(cfg["codec_seed"])
    first = torch.randperm(s, generator=gen)[torch.arange(n_centroids) % s].to(dev)
    centroids = sample16[first].contiguous()
    sample = sample16.float()
    for _ in range(cfg["kmeans_iters"]):
        near = nat.token_compress(sample16, dim, centroids).long()
        sums = torch.zeros_like(sample[:1]).repeat(n_centroids, 1).index_add_(0, near, sample)
        norm = sums.norm(dim=1, keepdim=True)
        centroids = torch.where(norm > 0, sums / norm.clamp_min(1e-30), centroids.float()).to(torch.float16).contiguous()
    near = nat.token_compress(sample16, dim, centroids).long()
    res = (sample[:, :dim] - centroids[near][:, :dim].float()).reshape(-1)
    if res.numel() > QUANTILE_SAMPLE:
        res = res[torch.randint(res.numel(), (QUANTILE_SAMPLE,), generator=gen).to(dev)]      # seeded, with repeats: a sample of the coordinates
    q = torch.quantile(res, torch.tensor([0.25, 0.5, 0.75, 0.125, 0.375, 0.625, 0.875], device=dev))
    return TokenCodec(centroids, q[:3].contiguous(), q[3:].contiguous(), dim)
