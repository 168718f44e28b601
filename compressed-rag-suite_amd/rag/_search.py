"""The search of ONE device's rows and how exact its answer is: what ``VectorStore`` (per shard, per filter) and ``RetrievalEngine``
(per buffer set, captured into hipGraphs) both run.  ``search_certified`` is the only caller of crs::cosine_topk_cert,
crs::cosine_topk_large_cert and crs::escalate_exact; ``search_view`` serves any top_k on any view; the escalation policy, the list
length, the merge dispatch, the status-2 retry and the ``last_exactness`` tally (numpy only) are here once each."""
from __future__ import annotations

import logging
from dataclasses import dataclass

import numpy as np

from rag import _native as nat

logger = logging.getLogger(__name__)


@dataclass
class ShardView:
    """The rows of ONE device that a search runs over (tensors stay owned by the store / the caller)."""
    slab: object                 # cuda fp16 | int8 [>= n, pdim]
    scales: object               # cuda fp32 [>= n] (int8) or None
    shadow: object               # cuda fp32 [>= n, dim] or None (no fp32 re-rank then)
    n: int
    dim: int
    slab_type: int
    id_base: int = 0             # added to local rows: the shard's first global row
    row_err_max: float = -1.0    # tracked |stored row - fp32 row|_2 maximum (< 0: the analytic worst case)
    row_map: object = None       # cuda int64 [n]: local row -> sidecar row (None: identity)
    space: int = 0               # nat.SPACE_*: cosine, or rows stored for 'ip' / 'l2' (dim is then the STORED row's: d + 1 for l2)
    norm_scale: object = None    # cuda fp32 [1]: the store's R (spaces 'ip' / 'l2')

    def sidecar_rows(self, rows):
        """Local rows of a result (-1: empty slot) -> sidecar rows."""
        import torch
        return rows if self.row_map is None else torch.where(rows >= 0, self.row_map[rows.clamp(min=0)], rows)


class SearchBuffers:
    """What one certified search writes: scan workspace, certificate / escalation workspace, the k' candidates of the slab, the
    result lists and the per-query status.  A caller that replays the search from a graph fills every attribute once."""
    ws = exact_ws = cand_s = cand_i = out_s = out_i = status = None


def escalates(refine_exact, slab_type: int) -> bool:
    """refine_exact 'auto': fp16 slabs escalate unproven queries, int8 slabs stay empirical (rag/indexing.py docstring)."""
    return slab_type == nat.SLAB_F16 if refine_exact == 'auto' else bool(refine_exact)


def first_cap(exact_cap: int, top_k: int) -> int:
    """First length of the escalation's row list: exact_cap, and at least 4 x top_k above MAX_K (the list must hold the
    top_k rows and the band around the k-th)."""
    if top_k <= nat.MAX_K:
        return exact_cap
    return min(nat.EXACT_MAX_CAP, max(exact_cap, 4 * top_k))


def exact_workspace(nq: int, cap: int, device):
    import torch
    return torch.empty(nat.exact_workspace_bytes(nq, cap), dtype=torch.uint8, device=device)


def order(s, i, k: int):
    """(score desc, row asc) via two stable sorts; empty slots (row < 0) last; keep k."""
    import torch
    big = torch.iinfo(torch.int64).max
    o = torch.argsort(torch.where(i >= 0, i, big), dim=1, stable=True)
    s, i = torch.gather(s, 1, o), torch.gather(i, 1, o)
    o = torch.argsort(torch.where(i >= 0, s, float("-inf")), dim=1, descending=True, stable=True)[:, :k]
    return torch.gather(s, 1, o), torch.gather(i, 1, o)


def merge_lists(gs, gi, top_k: int):
    """The lists of G shards, stacked [G, nq, top_k] on one device -> the best top_k of their union per query."""
    if top_k <= nat.MAX_K:
        return nat.merge_topk(gs, gi, top_k)
    if top_k <= nat.MAX_K_CERT and gs.shape[0] <= nat.MERGE_SORTED_MAX_LISTS:
        return nat.merge_sorted(gs, gi, top_k)      # every shard's list arrives sorted (score desc, row asc): co-ranking
    nq = gs.shape[1]
    return order(gs.permute(1, 0, 2).reshape(nq, -1), gi.permute(1, 0, 2).reshape(nq, -1), top_k)


def search_certified(view: ShardView, q32, q16, k_scan: int, k_out: int, cap: int, escalate: bool, bufs: SearchBuffers = None):
    """q32: UNIT fp32 queries [nq, dim], q16: their scan block -> (scores [nq, k_out], rows + id_base [nq, k_out], status int32
    [nq]: 0 proven the fp32 top-k of all rows, 1 escalated to it (escalate off: unproven), 2 more rows in the band than `cap`).
    k_out <= MAX_K: the scan's k_scan candidates, their fp32 re-rank and the proof that no un-fetched row can reach the list, in
    one call; above, up to MAX_K_CERT: the partitioned over-fetch (64 candidates from each row chunk; k_scan unused).  Queries
    without proof are made exact on the device (one more sweep for them; a no-op launch otherwise).  Nothing waits."""
    v, b = view, bufs if bufs is not None else SearchBuffers()
    exact_ws = b.exact_ws if bufs is not None else exact_workspace(q32.shape[0], cap, q32.device)
    if k_out <= nat.MAX_K:
        s, i, status = nat.cosine_topk_cert(q32, q16, v.slab, v.shadow, v.n, v.dim, k_scan, k_out, v.row_err_max, exact_ws, cap,
                                            scales=v.scales, id_base=v.id_base, workspace=b.ws, cand_scores=b.cand_s,
                                            cand_ids=b.cand_i, out_scores=b.out_s, out_ids=b.out_i, status=b.status)
    else:
        s, i, status = nat.cosine_topk_large_cert(q32, q16, v.slab, v.shadow, v.n, v.dim, k_out, v.row_err_max, exact_ws, cap,
                                                  scales=v.scales, id_base=v.id_base, workspace=b.ws, out_scores=b.out_s,
                                                  out_ids=b.out_i, status=b.status)
    if escalate:
        nat.escalate_exact(q32, q16, v.slab, v.shadow, v.n, v.id_base, k_out, s, i, status, exact_ws, cap, scales=v.scales)
    return s, i, status


def topk_gemm(view: ShardView, q32, top_k: int):
    """top_k above the scan kernels' limit (the reference accepts any n_results, rag/indexing.py:152-153): all slab scores
    of a row block through the library's GEMM kernel (crs_gemm_f16, fp32 out), device top-k per block, order by two
    stable sorts (score desc, row asc).  int8 rows are widened per block.  With the fp32 shadow the slab pass over-fetches
    by half and the candidates are re-scored in fp32 by the library (crs::score_rows_f32) before the final order -- the
    over-fetch re-rank without a certificate (that exists for top_k <= MAX_K_CERT: this path serves larger top_k and
    stores without the shadow).  The guarantee is the weaker, empirical one:
    a band of near-identical rows wider than the over-fetch can leave the list off the fp32 ranking, so last_exactness
    counts every query of such a search unproven (mode 'rerank')."""
    import torch
    from rag._encoder import gemm_f16
    slab, scales, shadow, n, dev = view.slab, view.scales, view.shadow, view.n, view.slab.device
    q16 = nat.queries_to_f16(q32, nat.SLAB_F16)
    if q16.shape[1] != slab.shape[1]:            # int8 slabs pad rows to 256 elements
        q16 = torch.nn.functional.pad(q16, (0, slab.shape[1] - q16.shape[1]))
    nq = q32.shape[0]
    keep = min(n, top_k + max(64, top_k // 2)) if shadow is not None else top_k
    best_s = torch.empty((nq, 0), dtype=torch.float32, device=dev)
    best_i = torch.empty((nq, 0), dtype=torch.int64, device=dev)
    block = 1 << 16
    zero = torch.zeros((nq, min(block, n)), dtype=torch.float32, device=dev)
    for lo in range(0, n, block):
        hi = min(n, lo + block)
        w = slab[lo:hi] if scales is None else (slab[lo:hi].float() * scales[lo:hi, None]).half()
        sc = gemm_f16(q16, w.contiguous(), residual=zero[:, : hi - lo].contiguous(), mode=2)
        ts, ti = sc.topk(min(keep, hi - lo), dim=1)
        best_s, best_i = torch.cat([best_s, ts], 1), torch.cat([best_i, ti + lo], 1)
        if best_s.shape[1] > 4 * keep:
            best_s, best_i = order(best_s, best_i, keep)
    s, i = order(best_s, best_i, keep)
    if shadow is not None:
        qn = torch.nn.functional.normalize(q32, p=2, dim=1, eps=1e-12).contiguous()
        s, i = order(nat.score_rows_f32(qn, shadow, n, 0, i), i, top_k)
    if s.shape[1] < top_k:
        pad = top_k - s.shape[1]
        s = torch.nn.functional.pad(s, (0, pad), value=float("-inf"))
        i = torch.nn.functional.pad(i, (0, pad), value=-1)
    return s, i


def search_view(view: ShardView, q32, top_k: int, overfetch: int, cap: int, escalate: bool):
    """q32: fp32 [nq, dim] on the view's device, any norm -> (scores [nq, top_k], SIDECAR rows [nq, top_k], certificate status
    int32 [nq] or None where no certificate exists) there.  Nothing here waits for the device."""
    import torch
    nq = q32.shape[0]
    if view.n == 0:
        return (torch.full((nq, top_k), float("-inf"), dtype=torch.float32, device=q32.device),
                torch.full((nq, top_k), -1, dtype=torch.int64, device=q32.device), None)
    status = None
    if view.space != nat.SPACE_COSINE:
        # the same certified search over the transformed rows, then the space's own distances, computed from the
        # caller's queries and the recovered vectors and ordered (distance asc, row asc): the first array returned holds DISTANCES
        if view.shadow is None or top_k > nat.MAX_K_CERT:
            raise ValueError(f"a search in space 'ip' / 'l2' needs the fp32 shadow and top_k <= {nat.MAX_K_CERT}")
        qt, q16 = nat.queries_to_space(q32, view.space, view.slab_type, view.norm_scale)
        k_scan = nat.overfetch(nq, top_k, overfetch, view.n, view.slab_type) if top_k <= nat.MAX_K else top_k
        _, i, status = search_certified(view, qt, q16, k_scan, top_k, cap, escalate)
        s, i = nat.space_distances(q32, view.space, view.shadow, view.n, view.id_base, view.norm_scale, i)
    elif view.shadow is not None and top_k <= nat.MAX_K_CERT:
        q16 = nat.queries_to_f16(q32, view.slab_type)
        qn = torch.nn.functional.normalize(q32, p=2, dim=1, eps=1e-12).contiguous()
        k_scan = nat.overfetch(nq, top_k, overfetch, view.n, view.slab_type) if top_k <= nat.MAX_K else top_k
        s, i, status = search_certified(view, qn, q16, k_scan, top_k, cap, escalate)
    elif top_k > nat.MAX_K:
        s, i = topk_gemm(view, q32, top_k)
    else:
        s, i = nat.cosine_topk(nat.queries_to_f16(q32, view.slab_type), view.slab, view.n, view.dim, top_k,
                               slab_type=view.slab_type, scales=view.scales)
    return s, view.sidecar_rows(i), status


def resolve_overflow(first, search, cap: int, top_k: int):
    """The status-2 retry.  first = search(cap), already launched (a store launches every shard before it reads any status);
    search(cap) -> (scores, rows, status or None).  Reads the status -- the one host wait of a certified search -- and, while a
    query's band held more rows than the list (status 2) and the list can grow, repeats the search with four times the list.
    -> (scores, rows, status as numpy or None)."""
    s, i, status = first
    if status is None:
        return s, i, None
    st = status.cpu().numpy()
    while (st == 2).any() and cap < nat.EXACT_MAX_CAP:
        cap = min(nat.EXACT_MAX_CAP, cap * 4)
        s, i, status = search(cap)
        st = status.cpu().numpy()
    if (st == 2).any():
        logger.warning(f"{int((st == 2).sum())} queries have more than {nat.EXACT_MAX_CAP} rows within the error band of "
                       f"their top-{top_k} (near-identical chunks): their lists are the fp32 re-rank of the over-fetch, unproven")
    return s, i, st


def tally(status, nq: int, top_k: int, refined: bool, escalate: bool) -> dict:
    """The ``last_exactness`` dict of nq queries.  status: the int32 [nq] status of one shard, a list of them (a query counts
    once, by its worst shard), or None / empty (no shard had rows to search: nothing to miss).  Without escalation status 1
    is unproven.  mode 'slab' (no fp32 shadow: no fp32 claim, queries 0), 'rerank' (top_k > MAX_K_CERT: no proof, every query
    unproven), 'certificate' otherwise."""
    if not refined:
        return {"queries": 0, "certified": 0, "escalated": 0, "unproven": 0, "mode": "slab"}
    if top_k > nat.MAX_K_CERT:
        return {"queries": nq, "certified": 0, "escalated": 0, "unproven": nq, "mode": "rerank"}
    shards = [np.asarray(st) for st in (status if isinstance(status, (list, tuple)) else [status]) if st is not None]
    worst = np.maximum.reduce(shards) if shards else np.zeros(nq, dtype=np.int32)
    if not escalate:
        worst = np.where(worst == 1, 2, worst)
    return {"queries": nq, "certified": int((worst == 0).sum()), "escalated": int((worst == 1).sum()),
            "unproven": int((worst == 2).sum()), "mode": "certificate"}


def add_tallies(a: dict, b: dict) -> dict:        # two disjoint sets of queries of one search (batch after batch)
    return dict(a, **{key: a[key] + b[key] for key in ("queries", "certified", "escalated", "unproven")})


def retried_tally(batch: dict, retry: dict) -> dict:
    """batch: the tally of a batch whose status-2 queries (counted unproven there) were searched again, retry: the tally of that
    second search -> the batch's tally with those queries counted by their final status."""
    out = add_tallies(batch, retry)
    out["queries"] -= retry["queries"]
    out["unproven"] -= retry["queries"]
    return out
