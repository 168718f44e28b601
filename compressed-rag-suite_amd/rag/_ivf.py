"""The inverted-file index of a VectorStore (``vector_store.ivf``): spherical k-means over the fp16 slab, the rows of
every list as row numbers, and the search that probes ``nprobe`` lists per query with crs::ivf_topk (csrc/ivf_probe.hip).

The slab is neither permuted nor copied: ``assign`` (int32 [n], the list of every row) is the source of truth, ``list_offsets``
(int32 [nlist + 1]) and ``list_rows`` (int32 [n], rows grouped by list, ascending within a list) are derived from it by one
stable device sort.  The centroids are an fp16 unit slab [nlist, pdim] written by the store's row writer, so assigning rows is
the existing scan with k = 1 over that slab with the slab's own rows as the query block."""
from __future__ import annotations

import math

from . import _native as nat

KEYS = ("nlist", "nprobe", "train_rows", "iters", "seed", "min_rows")
ASSIGN_ROWS = 8192        # slab rows one assignment scan takes as its queries
DEFAULT_NPROBE = 8        # measured (profiles/ivf_bench.json): the smallest with Recall@10 within 0.01 of nprobe 64 on the clustered set


def parse_config(cfg) -> dict:
    """The ``ivf`` dict of a store's config with its types checked; unset keys stay None (resolved at build time)."""
    if not isinstance(cfg, dict):
        raise ValueError(f"ivf must be a dict of {KEYS}, got {cfg!r}")
    unknown = sorted(set(cfg) - set(KEYS))
    if unknown:
        raise ValueError(f"ivf: unknown keys {unknown}; known: {KEYS}")
    out = {key: (None if cfg.get(key) is None else int(cfg[key])) for key in KEYS}
    out["nprobe"] = check_nprobe(DEFAULT_NPROBE if out["nprobe"] is None else out["nprobe"])
    out["iters"] = 10 if out["iters"] is None else out["iters"]
    out["seed"] = 0 if out["seed"] is None else out["seed"]
    if out["nlist"] is not None and not 1 <= out["nlist"] <= nat.IVF_MAX_LISTS:
        raise ValueError(f"ivf nlist must be in 1..{nat.IVF_MAX_LISTS}, got {out['nlist']}")
    if out["iters"] < 1:
        raise ValueError(f"ivf iters must be >= 1, got {out['iters']}")
    return out


def check_nprobe(nprobe) -> int:
    if not isinstance(nprobe, int) or isinstance(nprobe, bool) or not 1 <= nprobe <= nat.IVF_MAX_PROBE:
        raise ValueError(f"nprobe must be an integer in 1..{nat.IVF_MAX_PROBE}, got {nprobe!r}")
    return nprobe


def resolve_nlist(cfg: dict, count: int) -> int:
    """cfg's nlist, else the power of two nearest 4 sqrt(count)."""
    if cfg["nlist"] is not None:
        return cfg["nlist"]
    want = 4.0 * math.sqrt(max(count, 1))
    lo = 1 << max(0, int(math.floor(math.log2(want))))
    return min(nat.IVF_MAX_LISTS, lo if want - lo <= 2 * lo - want else 2 * lo)


def min_rows(cfg: dict, count: int) -> int:
    return cfg["min_rows"] if cfg["min_rows"] is not None else 32 * resolve_nlist(cfg, count)


class IvfIndex:
    """Centroids and lists over the first ``n_rows`` rows of one fp16 shard."""

    def __init__(self, cfg: dict, sh):
        import torch
        self.nlist = min(resolve_nlist(cfg, sh.n), sh.n)
        self.dim = sh.dim
        self.n_rows = 0
        self.assign = torch.empty(0, dtype=torch.int32, device=sh.device)
        self.centroids = torch.zeros((self.nlist, sh.pdim), dtype=torch.float16, device=sh.device)
        self._train(cfg, sh)
        self.extend(sh)

    def _nearest(self, rows16):
        """The nearest centroid of fp16 unit rows [m, pdim] (slab rows are query blocks as they are): int64 [m]."""
        import torch
        out = torch.empty(rows16.shape[0], dtype=torch.int64, device=rows16.device)
        for r0 in range(0, rows16.shape[0], ASSIGN_ROWS):
            _, best = nat.cosine_topk(rows16[r0:r0 + ASSIGN_ROWS], self.centroids, self.nlist, self.dim, 1)
            out[r0:r0 + ASSIGN_ROWS] = best[:, 0]
        return out

    def _train(self, cfg: dict, sh) -> None:
        """Spherical k-means on a seeded sample: assign by the scan, update by index_add_ + the row writer's normalisation.  An
        empty cluster is re-seeded with the sample row of the largest cluster that lies furthest from that cluster's centroid
        (ties: the lowest sample row), so a run is a function of the rows and the seed."""
        import torch
        gen = torch.Generator(device="cpu").manual_seed(cfg["seed"])
        want = cfg["train_rows"] if cfg["train_rows"] is not None else 256 * self.nlist
        m = max(self.nlist, min(sh.n, want))
        pick = torch.randperm(sh.n, generator=gen)[:m].to(sh.device)      # its first nlist rows are the initial centroids
        sample16 = sh.slab[pick]
        sample = sample16[:, :self.dim].float()
        nat.slab_append_f32(sample[:self.nlist].contiguous(), self.centroids, 0, nat.SLAB_F16)
        for _ in range(cfg["iters"]):
            near = self._nearest(sample16)
            sums = torch.zeros((self.nlist, self.dim), dtype=torch.float32, device=sh.device).index_add_(0, near, sample)
            sizes = torch.bincount(near, minlength=self.nlist)
            for empty in (sizes == 0).nonzero().flatten().tolist():
                big = int(sizes.argmax())
                members = (near == big).nonzero().flatten()
                fit = sample[members] @ (sums[big] / sums[big].norm().clamp_min(1e-30))
                far = members[int(fit.argmin())]
                sums[big] -= sample[far]
                sums[empty] = sample[far]
                near[far] = empty
                sizes[big] -= 1
                sizes[empty] = 1
            nat.slab_append_f32(sums.contiguous(), self.centroids, 0, nat.SLAB_F16)      # the writer normalises every row

    def extend(self, sh) -> None:
        """Assign the rows that arrived since (all of them after training) and re-derive the lists; the centroids stay."""
        import torch
        if sh.n > self.n_rows:
            new = self._nearest(sh.slab[self.n_rows:sh.n]).to(torch.int32)
            self.assign = torch.cat([self.assign, new])
            self.n_rows = sh.n
        order = torch.sort(self.assign, stable=True)
        self.list_rows = order.indices.to(torch.int32)
        sizes = torch.bincount(self.assign, minlength=self.nlist)
        self.list_offsets = torch.cat([sizes.new_zeros(1), sizes.cumsum(0)]).to(torch.int32)
        self.sizes_host = sizes.cpu().numpy()      # workspace sizing and get_stats

    def topk(self, q32, sh, top_k: int, nprobe: int, overfetch: int):
        """q32 fp32 [nq, dim] on the shard's device -> (scores fp32, rows int64) [nq, top_k] there: coarse search over the
        centroids, probe of the nprobe nearest lists at k' = 32 (64 when the re-rank's over-fetch asks for more), and with an
        fp32 shadow the candidates re-scored against it and ordered."""
        import torch
        from . import _search
        qn = torch.nn.functional.normalize(q32, p=2, dim=1, eps=1e-12).contiguous()
        q16 = nat.queries_to_f16(qn)
        nprobe = min(nprobe, self.nlist)
        kp = 32 if overfetch <= 32 else 64
        k = kp if sh.shadow is not None else top_k      # every candidate the probe kept goes to the re-rank
        out_s, out_r = [], []
        for q0 in range(0, q16.shape[0], nat.IVF_MAX_QUERIES):
            part = q16[q0:q0 + nat.IVF_MAX_QUERIES]
            _, lists = nat.cosine_topk(part, self.centroids, self.nlist, self.dim, nprobe)
            s, r = nat.ivf_topk(part, sh.slab, sh.n, self.dim, self.list_offsets, self.list_rows, lists.to(torch.int32), k, kp)
            out_s.append(s)
            out_r.append(r)
        s, r = torch.cat(out_s), torch.cat(out_r)
        if sh.shadow is None:
            return s, r
        return _search.order(nat.score_rows_f32(qn, sh.shadow, sh.n, 0, r), r, top_k)
