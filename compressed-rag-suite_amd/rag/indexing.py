"""Vector store: a flat, HBM-resident fp16 / int8 slab searched exactly on the MI355X.

Drop-in for the reference's ChromaDB-backed ``VectorStore`` (/root/reference/rag/indexing.py:14-211):
same constructor config keys, same method names, argument meaning, return shapes and exceptions.
What changed underneath: ``collection.add`` -> one ``crs::slab_append`` launch per batch (rows are
L2-normalised, cast to fp16 or int8+scale and appended to a device slab); ``collection.query`` ->
``crs::cosine_topk`` (exact brute-force scan + top-k; include/crs_hip.h, csrc/torch_ops.cpp).  Documents,
ids and metadata stay on the host, indexed by row.

New, additive surface (all keys absent from the reference config.json default so that it works unmodified):
  ``search_batch``            many queries per launch
  ``index_dtype``             'fp16' (default) | 'int8' (per-row scale)
  ``refine_fp32``             (default ON) keep an fp32 shadow of the rows (4 x dim bytes per row beside the fp16 / int8
                              slab), over-fetch ``refine_overfetch`` (24; 16 on shards below 4 M rows; at least 1.6 x top_k
                              above top_k 10: nat.overfetch) candidates and re-rank them in fp32: the ranking an
                              fp32 store such as the reference's returns (rag/indexing.py:114-119,171-176).  False = the
                              plain fp16 / int8 ranking, no shadow
  ``refine_exact``            'auto' (default) | True | False: every re-ranked list carries a per-query PROOF that it is the
                              fp32 top-k of all rows (crs::refine_f32_cert: k-th fp32 score > k'-th slab score + a measured
                              error bound); unproven queries (near-ties deeper than the over-fetch, e.g. near-duplicate
                              chunks) are escalated on the device (crs::escalate_exact: one more sweep lists every row that
                              can still rank, fp32 re-rank of the list).  'auto' escalates on fp16 slabs; on int8 slabs the
                              bound (~1e-2 for 768-d rows) is wider than typical score gaps, so the certificate rarely
                              holds and escalating would cost a second sweep for most batches: int8 stays
                              EMPIRICAL (re-rank only) unless refine_exact=True.  ``last_exactness`` reports the counts
                              of the last search and its mode (top_k > 1024: re-rank without proof, counted unproven)
  ``space``                   'cosine' (default) | 'ip' | 'l2': ChromaDB's hnsw:space, reported by ``collection.metadata``.  The scan is the
                              cosine scan in all three: an 'ip' / 'l2' store does NOT normalise its rows, it stores them divided by one
                              power of two R >= every row norm seen ('l2': by 2R, plus one coordinate |v|^2, so a 384-d collection
                              scans 512-element rows), converts queries to match (crs::queries_to_space) and, once the certified list
                              exists, computes ChromaDB's distance -- 1 - <q, x>, or sum (q - x)^2 -- in fp32 from the caller's own
                              vectors and orders the list by (distance, row) (crs::space_distances).  Certificate, escalation and
                              ``last_exactness`` mean what they mean for cosine; top_k up to 1024; dimensions up to 1023 ('l2').
                              ('l2' over rows whose norms spread widely amplifies the slab's error by 4 R^2: on 1 M isotropic rows
                              every query escalated at a log-normal sigma of 0.25 and came back UNPROVEN at 0.5 -- DESIGN 3.12.)  An
                              add or update whose largest norm exceeds R doubles R as needed and rescales the stored rows exactly
                              (crs::slab_rescale_space), so the store equals, bit for bit, one that was given all rows at once;
                              ``rows_f32`` returns the caller's vectors.  Vectors with a non-finite norm raise ValueError before
                              anything is written; coordinates whose value divided by 2R leaves the fp32 normal range (|x_i| below
                              ~1e-38 R) are outside the bit-for-bit and exact-recovery guarantees.  Needs the fp32 shadow
                              (refine_fp32: False raises) and ONE device (sharded / num_gpus / devices raise NotImplementedError:
                              a shared R across ranks needs a collective); the throughput engine is not used (retrieve_batch embeds,
                              then calls search_batch's search)
  ``num_gpus`` / ``devices``  ONE process driving N devices: contiguous row shards, per-device scans, partial lists
                              copied to the first device and merged there -- RAGPipeline stays one object
  ``sharded``                 SPMD (one process per GPU, torch.distributed): each rank keeps a row shard; ONE RCCL
                              all-gather of the per-shard wire blocks + merge on every rank
  ``delete`` / ``update`` / ``upsert``   change ONE document without re-indexing (a ChromaDB collection offers the three; the
                              reference never calls them, so the semantics are this module's):
                                delete(ids, where, where_document) -> rows removed: rows whose id is in ``ids`` AND that pass the
                                  filters; unknown ids ignored, an id several rows carry removes them all.  The shard's arrays
                                  are compacted IN PLACE and in order on the device (crs::slab_compact: a bounce buffer of at
                                  most 256 MB, no second copy, same data_ptr and capacity), so the store afterwards is, row for
                                  row, the store a fresh index of the survivors would be -- search results are bit-identical
                                update(ids, embeddings, documents, metadatas): per id, replace what is given (crs::slab_write_rows:
                                  the append's per-row function, same bits as an append); the metadata dict is replaced WHOLE,
                                  not merged key by key as ChromaDB does.  Unknown / ambiguous / repeated ids raise ValueError
                                  before anything changes
                                upsert(chunks, embeddings, metadata_fields): create_index's signature; known chunk ids are
                                  updated in place, the others appended in their given order
                              ``mutation_epoch`` counts the calls that changed something.  With persist_directory each such call
                              rewrites the files as a new generation (O(index) disk I/O: batch ids into one call)
  ``rerank_lexical``          the post-search half of ContextRetriever.retrieve_batch (score, similarity_threshold, the
                              token-overlap re-rank and its stable sort) for many result lists in one launch (csrc/rerank.hip), bit
                              for bit the host rule; the retriever's opt-in ``lexical_rerank: 'device'`` calls it.  It needs the
                              token ids of every chunk: a vocabulary (str -> int, exact, first-seen order) and a CSR of each row's
                              sorted distinct ids (SlabCollection._token_csr), derived data built by ONE Python pass over the
                              documents on first use, extended as rows arrive, dropped when a document changes, and mirrored on the
                              first device at 4 bytes per distinct token per chunk (+ 8 bytes per row of offsets); the sidecars are
                              replicated on every layout, so it serves sharded and multi-device stores alike
  ``bm25_rows`` / ``search_lexical_batch`` / ``fuse_rrf``   hybrid retrieval: an exact BM25 top-k over the whole collection (a flat
                              scan of the token CSR with its term frequencies and row lengths, csrc/bm25.hip) and the weighted
                              reciprocal rank fusion of a dense and a lexical list (csrc/fuse.hip); the retriever's opt-in
                              ``hybrid`` calls both.  The statistics share the token CSR's lifecycle (+ 4 bytes per distinct token
                              per chunk and 4 bytes per row on the first device)
  ``near_duplicates`` / ``duplicate_of`` / ``deduplicate`` / ``dedup_threshold``   exact near-duplicate detection: every pair of
                              rows whose cosine is at least a threshold, each pair once -- a thresholded self-join of the slab on
                              the matrix cores (csrc/join.hip) at threshold - epsilon, then an fp32 check of the candidates against
                              the shadow, so the answer is the fp32 one: exactly {i < j : sim32(i, j) >= t}.
                              ``duplicate_of`` applies greedy keep-first in row order (keep_first), ``deduplicate`` removes the
                              marked rows through delete's path.  Config key ``dedup_threshold`` (default None: nothing changes):
                              create_index joins all rows x the new batch and drops the batch's near-duplicates (old rows are always
                              kept) before sidecars and files see them -- one O(batch) append of the survivors, no generation
                              rewrite, mutation_epoch does not move; ``last_dedup`` = {'added', 'dropped'} of the last call;
                              ``dedup_max_pairs`` (4 M) bounds the pairs such a join may list.  fp16 cosine stores with the fp32
                              shadow on one device: int8, 'ip' / 'l2', sharded / num_gpus / devices raise NotImplementedError,
                              refine_fp32: False raises ValueError
  ``attach_token_encoder`` / ``token_index`` / ``max_index_bytes``   late-interaction re-ranking (rag/late_interaction.py, the
                              retriever's opt-in ``late_interaction``): a per-token index of every chunk -- fp16 [n_tokens, dimp]
                              unit vectors on the device, grown by doubling, and int64 offsets [n_rows + 1] on the host and on the
                              device -- that crs_maxsim reads through lists of sidecar rows (csrc/maxsim.hip).  Derived data, handled
                              like the token CSR: built on first use (one encoder pass over every document), extended by the rows
                              that arrived since (rows already held are never re-encoded by an append), and DROPPED WHOLE by a
                              delete, a document update or an upsert that changes a document -- the next use re-encodes every
                              document, an O(index) encoder pass: batch such calls.  NOT persisted (a re-opened store rebuilds it on
                              first use) and ONE device only (sharded / num_gpus / devices raise NotImplementedError).  Before any
                              encoding the bytes the index would take (host-side token counts x dimp x 2) are compared with
                              ``max_index_bytes`` (config key; default: half the device's total memory): more raises ValueError
  ``attach_sparse_encoder`` / ``sparse_index`` / ``sparse_rows`` / ``search_sparse_batch``   learned sparse retrieval (rag/sparse.py, the
                              retriever's opt-in ``sparse_model``): per row the at most ``sparse_doc_terms`` (256) largest weights of
                              its SPLADE vector as a device CSR -- int64 offsets, int32 vocabulary ids, fp32 weights, grown by doubling
                              -- that crs_sparse_topk scans for the queries' own sparse vectors (csrc/sparse_scan.hip; at most
                              ``sparse_query_terms`` = 64 terms a query).  Derived data with the token index's life cycle: built on
                              first use, extended by appends, DROPPED WHOLE by a delete, a document update or an upsert, NOT persisted,
                              ONE device only; ``max_index_bytes`` is compared with rows x sparse_doc_terms x 8 before any encoding
                              and with the exact size after compaction
``where`` / ``where_document`` filters work on every layout (the sidecars are replicated; each shard scans the
allowed rows it owns).  ``top_k`` is unlimited as in the reference: up to 1024 a refined shard is over-fetched by
partition (64 candidates from each of up to 64 row chunks, crs::cosine_topk_large_cert) and certified like top_k <= 64;
above that, or without the fp32 shadow, the shard is scored by the library's GEMM kernel and selected with a device sort.

There is no CPU fallback: without a GPU or without the native libraries every search raises.
"""
from __future__ import annotations

import json
import logging
import os
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from rag.chunking import Chunk
from rag import _native as nat
from rag import _search, _shard

logger = logging.getLogger(__name__)

_EMPTY = {'ids': [[]], 'documents': [[]], 'metadatas': [[]], 'distances': [[]]}


class _Shard:
    """The rows one device holds: slab (+ scales, + fp32 shadow) and, per local row, the global sidecar row."""

    def __init__(self, index_dtype: str, refine_fp32: bool, device, space: int = nat.SPACE_COSINE):
        import torch
        self.index_dtype, self.refine_fp32, self.device = index_dtype, refine_fp32, device
        # hnsw:space 'ip' / 'l2' (module docstring): rows are stored scaled by R = norm_scale, the smallest power of two
        # >= every row norm seen, NOT normalised; an l2 row carries one more coordinate.  The kernels read R from the device scalar,
        # the host mirror decides when it grows (0.0: no row seen yet)
        self.space = space
        self.norm_scale = torch.zeros(1, dtype=torch.float32, device=device)
        self.norm_scale_host = 0.0
        self.sdim: Optional[int] = None  # coordinates of a stored row: dim, or dim + 1 (l2)
        # largest |stored row - fp32 row|_2 of this shard, raised by every crs::slab_append: the row term of the
        # exactness certificate (csrc/exact.hip).  Lives on the device; read back lazily (row_err_max()).
        self.row_err = torch.zeros(1, dtype=torch.float32, device=device)
        self._row_err_host = None
        self.dim: Optional[int] = None   # the caller's dimension
        self.pdim: Optional[int] = None
        self.n = 0
        self.capacity = 0
        self.slab = None               # torch [capacity, pdim] fp16 | int8
        self.scales = None             # torch [capacity] fp32 (int8 only)
        self.shadow = None             # torch [capacity, sdim] fp32 (refine_fp32 only)
        self.rows_global = None        # torch [capacity] int64: sidecar row of each local row
        self.identity = True           # rows_global[i] == i for every row (single shard, unsharded): no mapping needed

    @property
    def slab_type(self) -> int:
        return nat.SLAB_I8 if self.index_dtype == "int8" else nat.SLAB_F16

    def _grow(self, old, shape, dtype):
        import torch
        new = torch.zeros(shape, dtype=dtype, device=self.device)
        if old is not None and self.n:
            new[: self.n].copy_(old[: self.n])
        return new

    def reserve(self, rows: int, dim: int):
        import torch
        if self.dim is None:
            sdim = nat.space_row_dim(dim, self.space)
            if sdim > 1024:
                raise ValueError(f"Embedding dimension {dim} is too large for space 'l2' (at most 1023: a row stores one more coordinate)")
            self.dim, self.sdim, self.pdim = dim, sdim, nat.padded_dim(sdim, self.slab_type)
        elif dim != self.dim:
            raise ValueError(f"Embedding dimension {dim} doesn't match the index dimension {self.dim}")
        if rows <= self.capacity:
            return
        cap = max(rows, int(self.capacity * 1.5) + 1024)
        self.slab = self._grow(self.slab, (cap, self.pdim), torch.int8 if self.slab_type == nat.SLAB_I8 else torch.float16)
        if self.slab_type == nat.SLAB_I8:
            self.scales = self._grow(self.scales, (cap,), torch.float32)
        if self.refine_fp32:
            self.shadow = self._grow(self.shadow, (cap, self.sdim), torch.float32)
        self.rows_global = self._grow(self.rows_global, (cap,), torch.int64)
        self.capacity = cap

    def store_rows(self, emb, local_rows=None):
        """emb: fp32 [m, dim] on this device (contiguous) -> rows self.n.. (an append into reserved capacity), or the rows
        `local_rows` (int64 [m] on this device, distinct, < self.n), in the shard's own space.  One per-row device function is
        behind all of it, so an updated row equals the same vector appended bit for bit.  In the spaces 'ip' / 'l2' the caller
        (VectorStore._grow_scale) has made norm_scale cover emb."""
        kw = dict(scales=self.scales, shadow=self.shadow, row_err=self.row_err)
        if self.space == nat.SPACE_COSINE:
            if local_rows is None:
                nat.slab_append_f32(emb, self.slab, self.n, self.slab_type, **kw)
            else:
                nat.slab_write_rows_f32(emb, local_rows, self.slab, self.n, **kw)
        elif local_rows is None:
            nat.slab_append_space_f32(emb, self.space, self.norm_scale, self.slab, self.n, **kw)
        else:
            nat.slab_write_rows_space_f32(emb, local_rows, self.space, self.norm_scale, self.slab, self.n, **kw)
        self._row_err_host = None

    def append(self, emb, first_global_row: int):
        """emb: fp32 [m, dim] on this device (contiguous) -> m more rows; they are sidecar rows first_global_row.."""
        import torch
        m, dim = emb.shape
        self.reserve(self.n + m, dim)
        if m == 0:
            return
        with torch.cuda.device(self.device):
            self.store_rows(emb)
            self.rows_global[self.n: self.n + m] = torch.arange(first_global_row, first_global_row + m, device=self.device)
        if first_global_row != self.n:
            self.identity = False
        self.n += m

    def grow_scale(self, norm_max: float) -> bool:
        """Make R cover a batch whose largest row norm is norm_max (finite): when R has to grow from R to R 2^j, every stored row is
        rescaled by the exact power of two first (crs::slab_rescale_space: one launch), so that it equals the same vector stored
        under the new R bit for bit.  True when stored rows were rescaled."""
        import math
        import torch
        new = nat.norm_scale_for(norm_max)
        if new <= self.norm_scale_host:
            return False
        rescaled = False
        with torch.cuda.device(self.device):
            if self.norm_scale_host > 0.0 and self.n:
                shift = int(round(math.log2(new / self.norm_scale_host)))
                nat.slab_rescale_space(self.n, self.dim, self.space, shift, self.slab, self.shadow, scales=self.scales, row_err=self.row_err)
                self._row_err_host = None
                rescaled = True
            self.norm_scale.fill_(new)
        self.norm_scale_host = new
        return rescaled

    def row_err_max(self) -> float:
        """The tracked row error as a host float (one 4-byte D2H after an append, cached until the next one)."""
        if self._row_err_host is None:
            self._row_err_host = float(self.row_err.item())
        return self._row_err_host

    def exact_workspace(self, nq: int, cap: int):
        return _search.exact_workspace(nq, cap, self.device)

    def view(self) -> _search.ShardView:
        """These rows as a search sees them (the tensors are shared, not copied)."""
        return _search.ShardView(self.slab, self.scales, self.shadow, self.n, self.sdim, self.slab_type, 0, self.row_err_max(),
                                 None if (self.identity or not self.n) else self.rows_global[:self.n], self.space, self.norm_scale)


def survivor_rows(n: int, dead) -> np.ndarray:
    """Stable compaction restated on the host: the source row of every destination row after the sorted rows `dead` left
    [0, n) -- what crs::slab_compact computes per row (source = destination + dead rows below the source)."""
    keep = np.ones(int(n), dtype=bool)
    keep[np.asarray(dead, dtype=np.int64)] = False
    return np.flatnonzero(keep).astype(np.int64)


def renumber_rows(rows, dead) -> np.ndarray:
    """Sidecar rows after the sorted sidecar rows `dead` were removed: new = old - number of dead rows below it (rows must
    not be dead themselves).  The device does the same with one torch.searchsorted per shard."""
    rows = np.asarray(rows, dtype=np.int64)
    return rows - np.searchsorted(np.asarray(dead, dtype=np.int64), rows, side="left")


def compact_windows(n_rows: int, m: int, window_rows: int, first_row: int = 0):
    """The destination windows [d0, d0 + w) crs::slab_compact walks for n_rows rows, m of them dead, W rows per window and the
    first dead row at or above first_row: whole multiples of W from the window holding first_row up to the n_rows - m survivors."""
    n_out, W = int(n_rows) - int(m), int(window_rows)
    if m <= 0 or n_out <= 0 or W <= 0:
        return []
    return [(d0, min(W, n_out - d0)) for d0 in range(int(first_row) // W * W, n_out, W)]


def keep_first(n: int, rows_a, rows_b) -> np.ndarray:
    """Greedy keep-first over a list of near-duplicate pairs (a < b; any order): int64 [n], entry r = -1 for a kept row, otherwise
    the kept row r duplicates.  Rows are visited in row order; row j is dropped iff some KEPT i < j forms a pair with it, and its
    entry is the smallest such i.  Not the transitive closure: of a chain a~b~c with a !~ c, b is dropped (for a) and c is kept,
    because its only partner b is gone.  A row that is no pair's second row is always kept."""
    dup = np.full(int(n), -1, dtype=np.int64)
    a = np.asarray(rows_a, dtype=np.int64)
    b = np.asarray(rows_b, dtype=np.int64)
    if a.size == 0:
        return dup
    if a.shape != b.shape or np.any(a >= b) or a.min() < 0 or b.max() >= n:
        raise ValueError("pairs must be (a, b) with 0 <= a < b < n")
    order = np.lexsort((a, b))                        # by b, then a: a row's partners are contiguous and ascending
    a, b = a[order].tolist(), b[order].tolist()
    for i, j in zip(a, b):
        if dup[j] < 0 and dup[i] < 0:                 # j still kept, i kept (final: i < j was decided before j's group began)
            dup[j] = i
    return dup


class _TokenCSR:
    """The token ids of every sidecar row, for the device's lexical re-rank: `vocab` str -> int32 id (ids in first-seen order,
    exact: no hashing), and per row the sorted distinct ids of set(document.lower().split()) -- the set ContextRetriever._tokens_of
    builds -- as a CSR: offsets int64 [rows + 1], token_ids int32 [total].  The host arrays and their device mirror grow
    geometrically; extend() tokenises only the new rows and device() uploads only what the mirror lacks.

    Beside them, filled by the same pass, the statistics BM25 needs (VectorStore.bm25_rows, csrc/bm25.hip): `tfs` int32 parallel to
    token_ids (occurrences of that token in that row), `doc_len` int32 [rows] (len(document.lower().split())), `df` int64
    [len(vocab)] (rows that hold the token) and `total_len` (the sum of doc_len); device_stats() mirrors tfs and doc_len like
    device() mirrors the ids."""

    def __init__(self):
        self.vocab: Dict[str, int] = {}
        self.rows = 0                      # rows tokenised so far
        self.total = 0                     # token ids they hold
        self._offsets = np.zeros(1024, dtype=np.int64)
        self._tokens = np.zeros(8192, dtype=np.int32)
        self._dev = None                   # (device, offsets tensor, tokens tensor)
        self._dev_rows, self._dev_total = 0, 0
        self.total_len = 0                 # sum of doc_len
        self._tfs = np.zeros(8192, dtype=np.int32)
        self._doc_len = np.zeros(1024, dtype=np.int32)
        self._df = np.zeros(1024, dtype=np.int64)
        self._dev_st = None                # (device, tfs tensor, doc_len tensor)
        self._dev_st_rows, self._dev_st_total = 0, 0

    @property
    def offsets(self) -> np.ndarray:
        return self._offsets[: self.rows + 1]

    @property
    def token_ids(self) -> np.ndarray:
        return self._tokens[: self.total]

    @property
    def tfs(self) -> np.ndarray:
        return self._tfs[: self.total]

    @property
    def doc_len(self) -> np.ndarray:
        return self._doc_len[: self.rows]

    @property
    def df(self) -> np.ndarray:
        return self._df[: len(self.vocab)]

    def row(self, r: int) -> np.ndarray:
        return self._tokens[self._offsets[r]: self._offsets[r + 1]]

    @staticmethod
    def _grown(arr, need: int):
        if need <= arr.shape[0]:
            return arr
        new = np.zeros(max(need, arr.shape[0] * 3 // 2), dtype=arr.dtype)
        new[: arr.shape[0]] = arr
        return new

    def extend(self, documents: Sequence[str]) -> None:
        """Tokenise documents[self.rows:] (the rows that arrived since the last call)."""
        vocab = self.vocab
        fresh, counts_of, n_words = [], [], []
        for doc in documents[self.rows:]:
            words = doc.lower().split()
            counts: Dict[int, int] = {}
            for w in words:
                t = vocab.setdefault(w, len(vocab))
                counts[t] = counts.get(t, 0) + 1
            ids = sorted(counts)
            fresh.append(ids)
            counts_of.append([counts[t] for t in ids])
            n_words.append(len(words))
        if not fresh:
            return
        if len(vocab) > 0x7fffffff:
            raise ValueError("more than 2^31 - 1 distinct tokens")
        lens = np.fromiter((len(ids) for ids in fresh), dtype=np.int64, count=len(fresh))
        added = int(lens.sum())
        self._offsets = self._grown(self._offsets, self.rows + len(fresh) + 1)
        self._tokens = self._grown(self._tokens, self.total + added)
        self._tfs = self._grown(self._tfs, self.total + added)
        self._doc_len = self._grown(self._doc_len, self.rows + len(fresh))
        self._df = self._grown(self._df, len(vocab))
        self._offsets[self.rows + 1: self.rows + len(fresh) + 1] = self.total + np.cumsum(lens)
        flat = np.fromiter((t for ids in fresh for t in ids), dtype=np.int32, count=added)
        self._tokens[self.total: self.total + flat.size] = flat
        self._tfs[self.total: self.total + flat.size] = np.fromiter((c for cs in counts_of for c in cs), dtype=np.int32, count=added)
        self._doc_len[self.rows: self.rows + len(fresh)] = n_words
        if added:
            self._df[: len(vocab)] += np.bincount(flat, minlength=len(vocab))      # ids are distinct within a row: one per row
        self.total_len += int(sum(n_words))
        self.rows += len(fresh)
        self.total += int(flat.size)

    def query_ids(self, query: str):
        """(sorted known ids of set(query.lower().split()), max(len(that set), 1)): the re-rank's `wanted` and `norm`."""
        wanted = set(query.lower().split())
        vocab = self.vocab
        return sorted(vocab[w] for w in wanted if w in vocab), max(len(wanted), 1)

    def device(self, device):
        """(offsets int64 [rows + 1], token_ids int32 [total]) on `device`: views of a mirror that only ever receives the tail
        the host gained since the last call (a larger mirror is allocated, and the old one copied on the device, when it is full)."""
        import torch
        if self._dev is None or self._dev[0] != device:
            self._dev = (device, torch.zeros(self._offsets.shape[0], dtype=torch.int64, device=device),
                         torch.zeros(self._tokens.shape[0], dtype=torch.int32, device=device))
            self._dev_rows, self._dev_total = 0, 0
        _, off, tok = self._dev
        if off.shape[0] < self.rows + 1 or tok.shape[0] < self.total:
            new_off = torch.zeros(self._offsets.shape[0], dtype=torch.int64, device=device)
            new_tok = torch.zeros(self._tokens.shape[0], dtype=torch.int32, device=device)
            new_off[: self._dev_rows + 1].copy_(off[: self._dev_rows + 1])
            new_tok[: self._dev_total].copy_(tok[: self._dev_total])
            off, tok = new_off, new_tok
            self._dev = (device, off, tok)
        if self._dev_rows < self.rows:
            off[self._dev_rows + 1: self.rows + 1].copy_(torch.from_numpy(self._offsets[self._dev_rows + 1: self.rows + 1]))
            if self._dev_total < self.total:
                tok[self._dev_total: self.total].copy_(torch.from_numpy(self._tokens[self._dev_total: self.total]))
            self._dev_rows, self._dev_total = self.rows, self.total
        return off[: self.rows + 1], tok[: self.total]

    def device_stats(self, device):
        """(tfs int32 [total], doc_len int32 [rows]) on `device`: the mirror of the BM25 statistics, with device()'s discipline
        (only the tail the host gained since the last call is uploaded; a full mirror is replaced by a larger one, copied on the
        device)."""
        import torch
        if self._dev_st is None or self._dev_st[0] != device:
            self._dev_st = (device, torch.zeros(self._tfs.shape[0], dtype=torch.int32, device=device),
                            torch.zeros(self._doc_len.shape[0], dtype=torch.int32, device=device))
            self._dev_st_rows, self._dev_st_total = 0, 0
        _, tf, dl = self._dev_st
        if tf.shape[0] < self.total or dl.shape[0] < self.rows:
            new_tf = torch.zeros(self._tfs.shape[0], dtype=torch.int32, device=device)
            new_dl = torch.zeros(self._doc_len.shape[0], dtype=torch.int32, device=device)
            new_tf[: self._dev_st_total].copy_(tf[: self._dev_st_total])
            new_dl[: self._dev_st_rows].copy_(dl[: self._dev_st_rows])
            tf, dl = new_tf, new_dl
            self._dev_st = (device, tf, dl)
        if self._dev_st_rows < self.rows:
            dl[self._dev_st_rows: self.rows].copy_(torch.from_numpy(self._doc_len[self._dev_st_rows: self.rows]))
            if self._dev_st_total < self.total:
                tf[self._dev_st_total: self.total].copy_(torch.from_numpy(self._tfs[self._dev_st_total: self.total]))
            self._dev_st_rows, self._dev_st_total = self.rows, self.total
        return tf[: self.total], dl[: self.rows]


class _TokenIndex:
    """The late-interaction token vectors of every row, for crs_maxsim (csrc/maxsim.hip): ``tok16`` cuda fp16 [capacity, dimp],
    the first ``n_tokens`` rows in use (row r's tokens are [offsets[r], offsets[r + 1])), grown by doubling; ``offsets`` int64
    [n_rows + 1] on the host, ``offsets_dev`` its device copy.  Extended in place as rows arrive: an append encodes the new rows
    alone."""

    def __init__(self, encoder, device):
        self.encoder, self.device, self.dimp = encoder, device, encoder.dimp
        self.tok16 = None
        self.n_tokens = 0
        self.offsets = np.zeros(1, dtype=np.int64)
        self.offsets_dev = None

    @property
    def n_rows(self) -> int:
        return len(self.offsets) - 1

    def extend(self, documents: Sequence[str], max_bytes: int) -> None:
        """Encode documents[n_rows:] and append their token vectors; ValueError (before any encoding) when the tokens in use would
        then take more than max_bytes.  The new rows are tokenised once and encoded straight into `tok16` (no temporary copy of
        them).  Memory beyond the guarded figure: the capacity grows by doubling, but never past max_bytes' worth of tokens unless
        the tokens in use need it, so the array itself stays within max(max_bytes, bytes in use); WHILE it grows the old and the
        new array exist side by side, so the peak of an append that grows an index of b bytes to capacity c is b + c, up to
        b + max_bytes; and the encoder's own workspace and hidden states of one batch come on top.  With the default limit of
        half the device's memory an index close to the limit can therefore still run out of memory when it grows: build it in
        one call (one allocation of the exact size) or set max_index_bytes lower."""
        import torch
        new = list(documents[self.n_rows:])
        if not new and self.offsets_dev is not None:
            return
        ids = self.encoder.tokenize_docs(new)
        counts = self.encoder.doc_token_counts(new, ids=ids)
        total = self.n_tokens + int(counts.sum())
        need = total * self.dimp * 2
        if need > max_bytes:
            raise ValueError(f"the late-interaction token index would take {need} bytes ({total} tokens x {self.dimp} x 2) for "
                             f"{len(documents)} rows, more than max_index_bytes = {int(max_bytes)}")
        with torch.cuda.device(self.device):
            held = self.tok16.shape[0] if self.tok16 is not None else 0
            if new and total > held:
                cap = max(total, min(2 * held, int(max_bytes) // (self.dimp * 2)), 1)
                grown = torch.zeros((cap, self.dimp), dtype=torch.float16, device=self.device)
                if self.n_tokens:
                    grown[:self.n_tokens] = self.tok16[:self.n_tokens]
                self.tok16 = grown
            if new:
                self.encoder.encode_docs_device(new, ids=ids, out=self.tok16, first_slot=self.n_tokens)
                self.offsets = np.concatenate([self.offsets, self.n_tokens + np.cumsum(counts)]).astype(np.int64)
                self.n_tokens = total
            if self.tok16 is None:
                self.tok16 = torch.zeros((1, self.dimp), dtype=torch.float16, device=self.device)
            self.offsets_dev = torch.from_numpy(self.offsets).to(self.device)


class _SparseIndex:
    """The learned-sparse vectors of every row as a device CSR, for crs_sparse_topk (csrc/sparse_scan.hip): ``tokens`` cuda int32 /
    ``weights`` cuda fp32 [capacity], the first ``n_terms`` entries in use (row r's terms are [offsets[r], offsets[r + 1]), ascending
    vocabulary ids), grown by doubling; ``offsets`` int64 [n_rows + 1] on the host, ``offsets_dev`` its device copy.  Extended in
    place as rows arrive: an append encodes the new rows alone."""

    GROUP = 4096          # documents encoded and compacted at a time: bounds the padded [GROUP, max_terms] block beside the index

    def __init__(self, encoder, device, max_terms: int):
        self.encoder, self.device, self.max_terms = encoder, device, int(max_terms)
        self.tokens = self.weights = None
        self.n_terms = 0
        self.offsets = np.zeros(1, dtype=np.int64)
        self.offsets_dev = None

    @property
    def n_rows(self) -> int:
        return len(self.offsets) - 1

    def extend(self, documents: Sequence[str], max_bytes: int) -> None:
        """Encode documents[n_rows:] and append their terms.  ValueError BEFORE any encoding when the estimate -- the terms held
        plus max_terms for every new row, 8 bytes each -- exceeds max_bytes; the exact size is checked again after each group's
        compaction, before the arrays grow.  While they grow the old and the new arrays exist side by side."""
        import torch
        new = list(documents[self.n_rows:])
        if not new and self.offsets_dev is not None:
            return
        estimate = (self.n_terms + len(new) * self.max_terms) * 8
        if estimate > max_bytes:
            raise ValueError(f"the sparse index could take {estimate} bytes ({self.n_terms} terms held + {len(new)} new rows x "
                             f"{self.max_terms} terms, 8 bytes each), more than max_index_bytes = {int(max_bytes)}")
        with VectorStore._device_guard(self.device):
            for lo in range(0, len(new), self.GROUP):
                ids, w, counts = self.encoder.encode_docs_device(new[lo: lo + self.GROUP], self.max_terms)
                counts_h = counts.cpu().numpy().astype(np.int64)
                total = self.n_terms + int(counts_h.sum())
                if total * 8 > max_bytes:
                    raise ValueError(f"the sparse index would take {total * 8} bytes ({total} terms), more than max_index_bytes = "
                                     f"{int(max_bytes)}")
                held = self.tokens.shape[0] if self.tokens is not None else 0
                if total > held:
                    cap = max(total, min(2 * held, int(max_bytes) // 8), 1)
                    tokens = torch.zeros(cap, dtype=torch.int32, device=self.device)
                    weights = torch.zeros(cap, dtype=torch.float32, device=self.device)
                    if self.n_terms:
                        tokens[:self.n_terms] = self.tokens[:self.n_terms]
                        weights[:self.n_terms] = self.weights[:self.n_terms]
                    self.tokens, self.weights = tokens, weights
                keep = ids >= 0                                        # row-major: rows in order, ids ascending inside a row
                self.tokens[self.n_terms:total] = ids[keep]
                self.weights[self.n_terms:total] = w[keep]
                self.offsets = np.concatenate([self.offsets, self.n_terms + np.cumsum(counts_h)]).astype(np.int64)
                self.n_terms = total
            if self.tokens is None:
                self.tokens = torch.zeros(1, dtype=torch.int32, device=self.device)
                self.weights = torch.zeros(1, dtype=torch.float32, device=self.device)
            self.offsets_dev = torch.from_numpy(self.offsets).to(self.device)


class SlabCollection:
    """What ``VectorStore.collection`` exposes (the retriever reads ``.metadata`` and the harness ``.count()``,
    reference rag/retrieval.py:48-50).  Owns the per-device shards and the host sidecars."""

    def __init__(self, name: str, index_dtype: str, refine_fp32: bool, devices: Sequence, space: str = "cosine"):
        self.name = name
        self.metadata = {"hnsw:space": space}
        self.space = nat.SPACES[space]
        self.index_dtype = index_dtype
        self.refine_fp32 = refine_fp32
        self.shards: List[_Shard] = [_Shard(index_dtype, refine_fp32, d, self.space) for d in devices]
        self.ids: List[str] = []
        self.documents: List[str] = []
        self.metadatas: List[dict] = []

    @property
    def slab_type(self) -> int:
        return nat.SLAB_I8 if self.index_dtype == "int8" else nat.SLAB_F16

    # first-shard views (single-device stores: the whole index)
    @property
    def device(self):
        return self.shards[0].device

    @property
    def dim(self):
        return self.shards[0].dim

    @property
    def sdim(self):
        return self.shards[0].sdim

    @property
    def pdim(self):
        return self.shards[0].pdim

    @property
    def n(self) -> int:
        return sum(s.n for s in self.shards)

    @property
    def slab(self):
        return self.shards[0].slab

    @property
    def scales(self):
        return self.shards[0].scales

    @property
    def shadow(self):
        return self.shards[0].shadow

    def count(self) -> int:
        return len(self.ids)

    # -- one-document mutation, for callers who hold the collection as they would a ChromaDB one (VectorStore does the work)
    def _store(self):
        owner = self.__dict__.get("_owner")
        store = owner() if owner is not None else None
        if store is None or store.collection is not self:
            raise ValueError("this collection is no longer attached to a VectorStore")
        return store

    def delete(self, ids=None, where=None, where_document=None) -> int:
        return self._store().delete(ids=ids, where=where, where_document=where_document)

    def update(self, ids, embeddings=None, documents=None, metadatas=None) -> None:
        return self._store().update(ids, embeddings=embeddings, documents=documents, metadatas=metadatas)

    def upsert(self, chunks, embeddings, metadata_fields=None) -> None:
        return self._store().upsert(chunks, embeddings, metadata_fields=metadata_fields)

    def _id_rows(self):
        """id -> sidecar rows (a list: create_index accepts duplicate ids), built once and extended as rows arrive like
        _inverted; dropped by a delete (every row number above the first deleted row changes)."""
        idmap = self.__dict__.setdefault("_idmap", {})
        done = self.__dict__.get("_idmap_rows", 0)
        for row in range(done, len(self.ids)):
            idmap.setdefault(self.ids[row], []).append(row)
        self.__dict__["_idmap_rows"] = len(self.ids)
        return idmap

    def _drop_derived(self, ids_changed: bool, metadata_changed: bool = True, documents_changed: bool = True):
        """Forget what was derived from the sidecars: the inverted metadata index, (rows renumbered) the id map, and (a document
        changed, or rows renumbered) the token CSR with its device mirror, the late-interaction token index and the sparse index."""
        if metadata_changed or ids_changed:
            self.__dict__.pop("_inv", None)
            self.__dict__.pop("_inv_rows", None)
        if ids_changed:
            self.__dict__.pop("_idmap", None)
            self.__dict__.pop("_idmap_rows", None)
        if documents_changed or ids_changed:
            self.__dict__.pop("_tok", None)
            self.__dict__.pop("_li", None)       # the late-interaction token index: the next use re-encodes every document
            self.__dict__.pop("_sp", None)       # the learned-sparse index: likewise

    def _token_csr(self) -> _TokenCSR:
        """The token ids of every row (see _TokenCSR): built by one pass over the documents on first use, extended by the rows
        that arrived since, like _inverted / _id_rows; dropped by _drop_derived when a document changes or rows are renumbered."""
        csr = self.__dict__.get("_tok")
        if csr is None:
            csr = self.__dict__["_tok"] = _TokenCSR()
        if csr.rows < len(self.documents):
            csr.extend(self.documents)
        return csr

    def _token_index(self, encoder, max_bytes: int) -> _TokenIndex:
        """The late-interaction token vectors of every row (see _TokenIndex), for `encoder`: built on first use, extended by the
        rows that arrived since, like _token_csr; dropped by _drop_derived, and when another encoder asks."""
        index = self.__dict__.get("_li")
        if index is None or index.encoder is not encoder:
            index = self.__dict__["_li"] = _TokenIndex(encoder, self.device)
        if index.n_rows < len(self.documents) or index.offsets_dev is None:
            index.extend(self.documents, max_bytes)
        return index

    def _sparse_index(self, encoder, max_terms: int, max_bytes: int) -> _SparseIndex:
        """The learned-sparse vectors of every row (see _SparseIndex), for `encoder`: built on first use, extended by the rows that
        arrived since, like _token_index; dropped by _drop_derived, and when another encoder or term cap asks."""
        index = self.__dict__.get("_sp")
        if index is None or index.encoder is not encoder or index.max_terms != int(max_terms):
            index = self.__dict__["_sp"] = _SparseIndex(encoder, self.device, max_terms)
        if index.n_rows < len(self.documents) or index.offsets_dev is None:
            index.extend(self.documents, max_bytes)
        return index

    # -- metadata filters: value -> rows, built once and extended as rows arrive (the per-query loop over all metadatas is gone)
    def _inverted(self):
        inv = self.__dict__.setdefault("_inv", {})
        done = self.__dict__.get("_inv_rows", 0)
        for row in range(done, len(self.metadatas)):
            for key, val in self.metadatas[row].items():
                try:
                    inv.setdefault(key, {}).setdefault(val, []).append(row)
                except TypeError:           # unhashable value: never equal to a scalar filter value
                    pass
        self.__dict__["_inv_rows"] = len(self.metadatas)
        return inv

    def _where_rows(self, where: dict, n: int):
        """Rows passing a ChromaDB `where` document: {key: value | {op: value}} (AND over keys), {"$and": [...]},
        {"$or": [...]}; ops $eq $ne $in $nin $gt $gte $lt $lte (chromadb 1.3.0's documented operators; the reference only
        forwards the dict).  Values are looked up in the inverted index: the cost follows the DISTINCT values of a key."""
        every = lambda: np.arange(n, dtype=np.int64)                                          # noqa: E731
        none = lambda: np.zeros(0, dtype=np.int64)                                            # noqa: E731
        rows_of = lambda col, v: np.asarray(col.get(v, []), dtype=np.int64)                   # noqa: E731
        out = None
        for key, want in where.items():
            if key in ("$and", "$or"):
                parts = [self._where_rows(w, n) for w in want]
                if key == "$and":
                    hit = every()
                    for p_ in parts:
                        hit = np.intersect1d(hit, p_, assume_unique=True)
                else:
                    hit = np.unique(np.concatenate(parts)) if parts else none()
            else:
                col = self._inverted().get(key, {})
                op, val = ("$eq", want)
                if isinstance(want, dict):
                    (op, val), = want.items()
                try:
                    if op in ("$eq", "$ne"):
                        if val is None:       # meta.get(key) == None: the rows WITHOUT the key
                            have = [np.asarray(v, dtype=np.int64) for v in col.values()]
                            eq = np.setdiff1d(every(), np.concatenate(have) if have else none())
                        else:
                            eq = rows_of(col, val)
                        hit = eq if op == "$eq" else np.setdiff1d(every(), eq, assume_unique=True)
                    elif op in ("$in", "$nin") and isinstance(val, (list, tuple)):
                        parts = [rows_of(col, v) for v in val]
                        inn = np.unique(np.concatenate(parts)) if parts else none()
                        hit = inn if op == "$in" else np.setdiff1d(every(), inn, assume_unique=True)
                    elif op in ("$gt", "$gte", "$lt", "$lte") and isinstance(val, (int, float)) and not isinstance(val, bool):
                        cmp = {"$gt": lambda x: x > val, "$gte": lambda x: x >= val, "$lt": lambda x: x < val, "$lte": lambda x: x <= val}[op]
                        parts = [np.asarray(r, dtype=np.int64) for v, r in col.items()
                                 if isinstance(v, (int, float)) and not isinstance(v, bool) and cmp(v)]
                        hit = np.sort(np.concatenate(parts)) if parts else none()
                    else:
                        hit = none()
                except TypeError:             # unhashable filter value: nothing can equal it
                    hit = every() if op in ("$ne", "$nin") else none()
            out = hit if out is None else np.intersect1d(out, hit, assume_unique=True)
        return every() if out is None else out

    def _doc_rows(self, cond: dict, base):
        rows = base
        for op, val in cond.items():
            if op == "$contains":
                rows = [r for r in rows if val in self.documents[r]]
            elif op == "$not_contains":
                rows = [r for r in rows if val not in self.documents[r]]
            elif op == "$and":
                for c in val:
                    rows = self._doc_rows(c, rows)
            elif op == "$or":
                keep = set()
                for c in val:
                    keep.update(self._doc_rows(c, rows))
                rows = [r for r in rows if r in keep]
        return rows

    def rows_matching(self, where: Optional[dict], where_document: Optional[dict]):
        """Sidecar rows (ascending numpy int64) that pass the filters the reference forwards to ChromaDB
        (rag/indexing.py:129-130,174).  None = no filter."""
        if not where and not where_document:
            return None
        n = len(self.ids)
        rows = self._where_rows(where, n) if where else np.arange(n, dtype=np.int64)
        if where_document:                    # substring tests have no index: one pass over the surviving documents
            rows = np.asarray(self._doc_rows(where_document, rows.tolist()), dtype=np.int64)
        return rows


class VectorStore:
    """Vector store on an HBM slab.  Handles storage, indexing and exact similarity search."""

    def __init__(self, config: dict):
        self.collection_name = config.get('collection_name', 'rag_documents')
        self.persist_directory = config.get('persist_directory', None)
        # additive knobs (absent from the reference config.json -> defaults)
        self.index_dtype = config.get('index_dtype', 'fp16')
        if self.index_dtype not in ('fp16', 'int8'):
            raise ValueError(f"index_dtype must be 'fp16' or 'int8', got {self.index_dtype!r}")
        refine = config.get('refine_fp32', 'auto')
        self.refine_fp32 = True if refine == 'auto' else bool(refine)
        self.space = config.get('space', 'cosine')
        if self.space not in nat.SPACES:
            raise ValueError(f"space must be 'cosine', 'ip' or 'l2', got {self.space!r}")
        if self.space != 'cosine' and not self.refine_fp32:
            raise ValueError(f"space {self.space!r} needs the fp32 shadow (the distances and the caller's vectors are recovered from it): "
                             "refine_fp32 must not be False")
        self.refine_overfetch = int(config.get('refine_overfetch', 24))
        exact = config.get('refine_exact', 'auto')
        if exact not in ('auto', True, False):
            raise ValueError(f"refine_exact must be 'auto', True or False, got {exact!r}")
        self.refine_exact = exact
        self.exact_cap = int(config.get('exact_cap', nat.EXACT_CAP))
        # certificate outcome of the most recent search, rewritten by every search: queries proven exact by the over-fetch
        # alone / escalated to exactness on the device / left unproven (escalation off, or a band of more than EXACT_MAX_CAP
        # near-identical rows).  mode: 'certificate' (fp32 re-rank + proof, top_k <= 1024; above 64 the over-fetch is partitioned,
        # nat.cosine_topk_large_cert), 'rerank' (top_k > 1024: fp32 re-rank of an over-fetch without proof, every query counted
        # unproven), 'slab' (refine_fp32=False: the slab's own ranking, no fp32 claim; queries 0)
        self.last_exactness = {"queries": 0, "certified": 0, "escalated": 0, "unproven": 0, "mode": None}
        self.sharded = bool(config.get('sharded', False))
        self._device = config.get('device', None)
        self._devices_cfg = config.get('devices', None)
        self.num_gpus = int(config.get('num_gpus', 0) or 0)
        if self.space != 'cosine':
            # one scale R is shared by every row: across ranks or devices that needs a collective
            for layout, on in (("sharded=True", self.sharded), ("num_gpus > 1", self.num_gpus > 1), ("devices", bool(self._devices_cfg))):
                if on:
                    raise NotImplementedError(f"space {self.space!r} is not supported with {layout}: the rows of such a store share one "
                                              "norm scale, which a single-device store keeps")
        # near-duplicate removal at index time (module docstring): None = nothing changes anywhere
        self.dedup_threshold = config.get('dedup_threshold', None)
        self.dedup_max_pairs = int(config.get('dedup_max_pairs', 1 << 22))
        self.last_dedup = {"added": 0, "dropped": 0}      # rows the last create_index kept / dropped as near-duplicates
        self.last_join = {"stripes": 0, "reruns": 0, "candidates": 0}   # of the last near-duplicate join
        self._join_stripe_rows = 1 << 18                  # rows per stripe edge: (2^18 / 256)^2 = 2^20 tile pairs per launch
        self._join_first_cap = 1 << 16                    # candidate slots a stripe is first given (it is re-run when they overflow)
        if self.dedup_threshold is not None:
            self.dedup_threshold = self._join_refusals(self.dedup_threshold)
        if self.sharded and (self.num_gpus > 1 or self._devices_cfg):
            raise ValueError("'sharded' (one process per GPU) and 'num_gpus'/'devices' (one process, N devices) are exclusive")
        if self.sharded and self.persist_directory:
            raise NotImplementedError("persist_directory is not supported with sharded=True (each rank holds only its rows); "
                                      "use num_gpus for a persisted multi-GPU store")
        # late-interaction token index (module docstring): the encoder comes through attach_token_encoder
        self.max_index_bytes = config.get('max_index_bytes', None)     # None: half the device's total memory, read on first use
        self._token_encoder = None
        # learned sparse retrieval (module docstring): the encoder comes through attach_sparse_encoder
        self._sparse_encoder = None
        self.sparse_doc_terms = int(config.get('sparse_doc_terms', 256))       # terms kept per document (<= SPARSE_MAX_TERMS)
        self.sparse_query_terms = int(config.get('sparse_query_terms', 64))    # terms kept per query: 64 x 64 = one launch's pair cap
        for name in ('sparse_doc_terms', 'sparse_query_terms'):
            if not 1 <= getattr(self, name) <= nat.SPARSE_MAX_TERMS:
                raise ValueError(f"{name} must be in 1..{nat.SPARSE_MAX_TERMS}, got {getattr(self, name)}")
        self.last_sparse = {'queries': 0, 'query_terms': 0, 'launches': 0}     # what the last sparse_rows call ran
        self._filters = {}      # filter key -> {"n": rows when built, "rows": allowed sidecar rows, "shards": {g: compacted sub-slab}}
        self._persisted_rows = None   # rows the append-only files hold (None: nothing / legacy format on disk)
        self._docs_bytes = 0          # length of the sidecar file the header vouches for
        self._gen = None              # generation of the files the header names (None: the un-suffixed names)
        self._gen_pending = False     # a generation rewrite failed: the memory is ahead of the files, the next persist rewrites
        self.mutation_epoch = 0       # +1 per delete / update / upsert that changed something
        self.client = self  # the reference keeps a chromadb client here; nothing else reads it
        self.collection: Optional[SlabCollection] = None
        self._wire = {}     # (nq, k) -> WireBlock (SPMD exchange buffers)
        self._initialize_collection()

    # -- helpers -------------------------------------------------------------------------------
    def _torch_devices(self):
        import torch
        nat.require_gpu()
        if self._devices_cfg:
            return [torch.device(d) for d in self._devices_cfg]
        if self.num_gpus > 1:
            have = torch.cuda.device_count()
            if self.num_gpus > have:
                raise nat.NativeError(f"num_gpus={self.num_gpus} but only {have} device(s) are visible")
            return [torch.device("cuda", g) for g in range(self.num_gpus)]
        if self._device is not None and str(self._device).startswith("cuda"):
            d = torch.device(self._device)
            return [d if d.index is not None else torch.device("cuda", torch.cuda.current_device())]
        return [torch.device("cuda", torch.cuda.current_device())]

    def _dist(self):
        if not self.sharded:
            return None
        import torch.distributed as dist
        return dist if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1 else None

    def _new_collection(self) -> SlabCollection:
        return self._adopt(SlabCollection(self.collection_name, self.index_dtype, self.refine_fp32, self._torch_devices(), self.space))

    def _adopt(self, col: SlabCollection) -> SlabCollection:
        import weakref
        col._owner = weakref.ref(self)        # collection.delete / update / upsert delegate to this store
        return col

    # -- persistence (the PersistentClient analogue, reference rag/indexing.py:32-34): APPEND-ONLY files, so that an add
    # costs O(batch), not O(index):
    #     <name>.meta.json    header {format, n, dim, pdim, index_dtype, shadow, row_err_max}; rewritten (tmp + rename) LAST;
    #                         + {space, norm_scale} when the space is not cosine (a cosine store's header is unchanged)
    #     <name>.slab.bin     rows [n, pdim] fp16 | int8, raw little-endian, in sidecar order
    #     <name>.scales.bin   fp32 [n]            (int8)
    #     <name>.shadow.bin   fp32 [n, dim]       (refine_fp32; space l2: [n, dim + 1], the rows as stored)
    #     <name>.docs.jsonl   one {"id", "document", "metadata"} line per row
    # The header's n is the truth: bytes or lines past it (a crash between the appends and the header) are ignored and
    # overwritten by the next add; files SHORTER than the header says mean corruption and raise.  The round-2 format
    # (<name>.slab.npz + <name>.docs.json, rewritten whole on every add) is still read.
    # GENERATIONS: delete / update / upsert change rows the files already hold, so they write the complete new set under new
    # names -- <name>.g<G>.slab.bin, .scales.bin, .shadow.bin, .docs.jsonl, each fsynced -- THEN replace the header (which
    # carries "gen": G), THEN remove the previous generation.  A crash before the header's rename leaves the old header and the
    # old files untouched: the store re-opens as it was before the call.  A header without "gen" names the un-suffixed files.
    # Appends continue into the current generation's files.  Cost: O(index) disk I/O per mutating call.
    _GEN_KEYS = ("slab", "scales", "shadow", "docs")

    def _persist_paths(self, gen="current"):
        base = os.path.join(self.persist_directory, self.collection_name)
        gen = self._gen if gen == "current" else gen
        sfx = f".g{int(gen)}" if gen else ""
        out = {k: base + ext for k, ext in (("meta", ".meta.json"), ("legacy_slab", ".slab.npz"), ("legacy_docs", ".docs.json"))}
        out.update({k: base + sfx + ext for k, ext in (("slab", ".slab.bin"), ("scales", ".scales.bin"),
                                                       ("shadow", ".shadow.bin"), ("docs", ".docs.jsonl"))})
        return out

    def _remove_other_generations(self, keep):
        """Remove the data files of every generation but `keep` (None: the un-suffixed names): the previous one, and whatever a
        crashed rewrite left behind."""
        import re
        pat = re.compile(re.escape(self.collection_name) + r"(?:\.g(\d+))?\.(?:slab\.bin|scales\.bin|shadow\.bin|docs\.jsonl)$")
        for name in os.listdir(self.persist_directory):
            hit = pat.fullmatch(name)
            if hit and (int(hit.group(1)) if hit.group(1) else None) != (int(keep) if keep else None):
                os.remove(os.path.join(self.persist_directory, name))

    def _load_rows_into(self, col, n, dim, rows, refine, row_err, norm_scale: float = 0.0):
        import torch
        for g, (lo, hi) in enumerate(_shard.batch_slices(n, len(col.shards))):
            sh = col.shards[g]
            sh.reserve(hi - lo, dim)
            if hi > lo:
                sh.slab[: hi - lo].copy_(torch.from_numpy(np.ascontiguousarray(rows["slab"][lo:hi])))
                if rows["scales"] is not None:
                    sh.scales[: hi - lo].copy_(torch.from_numpy(np.ascontiguousarray(rows["scales"][lo:hi])))
                if refine:
                    sh.shadow[: hi - lo].copy_(torch.from_numpy(np.ascontiguousarray(rows["shadow"][lo:hi])))
                sh.rows_global[: hi - lo] = torch.arange(lo, hi, device=sh.device)
            sh.n = hi - lo
            sh.identity = (lo == 0)
            sh.row_err.fill_(row_err)
            if col.space != nat.SPACE_COSINE:
                sh.norm_scale.fill_(norm_scale)
                sh.norm_scale_host = float(norm_scale)

    def _initialize_collection(self):
        """Re-open a persisted collection if there is one (reference: get_collection, :46-55)."""
        if not self.persist_directory:
            logger.info("Using in-memory (HBM) storage")
            return
        paths = self._persist_paths()
        legacy = not os.path.exists(paths["meta"])
        if legacy and not (os.path.exists(paths["legacy_slab"]) and os.path.exists(paths["legacy_docs"])):
            logger.info(f"Collection '{self.collection_name}' will be created on first add")
            return
        try:
            if legacy:
                z = np.load(paths["legacy_slab"], allow_pickle=False)
                with open(paths["legacy_docs"]) as fh:
                    side = json.load(fh)
                n, dim, dtype = int(z["n"]), int(z["dim"]), str(z["index_dtype"])
                rows = {"slab": z["slab"], "scales": z["scales"] if dtype == "int8" else None,
                        "shadow": z["shadow"] if "shadow" in z.files else None}
                row_err = float(z["row_err_max"]) if "row_err_max" in z.files else None
                ids, docs, metas = side["ids"], side["documents"], side["metadatas"]
                if len(ids) != n or rows["slab"].shape[0] != n:
                    raise ValueError(f"slab holds {rows['slab'].shape[0]} rows, sidecar {len(ids)}, header {n}")
            else:
                with open(paths["meta"]) as fh:
                    meta = json.load(fh)
                self._gen = int(meta["gen"]) if meta.get("gen") else None
                paths = self._persist_paths()
                n, dim, pdim, dtype = int(meta["n"]), int(meta["dim"]), int(meta["pdim"]), str(meta["index_dtype"])
                stored_space = str(meta.get("space", "cosine"))
                if stored_space not in nat.SPACES:
                    raise ValueError(f"unknown space {stored_space!r}")
                elem = np.int8 if dtype == "int8" else np.float16

                def raw(key, np_dtype, width):
                    need = n * width * np.dtype(np_dtype).itemsize
                    if os.path.getsize(paths[key]) < need:
                        raise ValueError(f"{os.path.basename(paths[key])} holds fewer than the header's {n} rows")
                    return np.fromfile(paths[key], dtype=np_dtype, count=n * width).reshape(n, width) if n else np.zeros((0, width), np_dtype)

                rows = {"slab": raw("slab", elem, pdim),
                        "scales": raw("scales", np.float32, 1).reshape(-1) if dtype == "int8" else None,
                        "shadow": raw("shadow", np.float32, nat.space_row_dim(dim, nat.SPACES[stored_space])) if meta.get("shadow") else None}
                row_err = meta.get("row_err_max")
                ids, docs, metas = [], [], []
                with open(paths["docs"], "rb") as fh:
                    blob = fh.read(int(meta["docs_bytes"]))
                if len(blob) < int(meta["docs_bytes"]):
                    raise ValueError("sidecar shorter than the header says")
                for line in blob.decode("utf-8").splitlines():
                    rec = json.loads(line)
                    ids.append(rec["id"]); docs.append(rec["document"]); metas.append(rec["metadata"])
                if len(ids) != n:
                    raise ValueError(f"sidecar holds {len(ids)} rows, header {n}")
                self._docs_bytes = int(meta["docs_bytes"])
        except Exception as e:
            # a truncated / foreign file must not silently become an empty store that the next add overwrites
            raise RuntimeError(f"persisted collection '{self.collection_name}' under {self.persist_directory} is unreadable: {e}") from e
        stored_space = "cosine" if legacy else stored_space
        if stored_space != self.space:
            raise ValueError(f"persisted collection '{self.collection_name}' was built with space {stored_space!r}; "
                             f"this store asks for {self.space!r}")
        if self.space != 'cosine' and rows["shadow"] is None:
            raise ValueError(f"persisted collection '{self.collection_name}' of space {self.space!r} has no fp32 shadow")
        self.index_dtype = dtype
        refine = self.refine_fp32 and rows["shadow"] is not None
        if self.refine_fp32 and not refine:
            logger.warning("persisted collection has no fp32 shadow; refine_fp32 disabled")
        col = self._adopt(SlabCollection(self.collection_name, dtype, refine, self._torch_devices(), self.space))
        # the certificate's row term: the persisted maximum, or the analytic worst case for files written before it existed
        if row_err is None:
            # (over the STORED row's coordinates: an l2 row has one more than the caller's dimension)
            row_err = nat.exact_row_error_bound(nat.space_row_dim(dim, nat.SPACES[self.space]),
                                                nat.SLAB_I8 if dtype == "int8" else nat.SLAB_F16)
        self._load_rows_into(col, n, dim, rows, refine, float(row_err), 0.0 if legacy else float(meta.get("norm_scale", 0.0)))
        col.ids, col.documents, col.metadatas = ids, docs, metas
        self.collection = col
        # appends continue the files only when they hold exactly what this store keeps (same shadow choice); else the next
        # add rewrites them once in the current format
        self._persisted_rows = n if (not legacy and bool(meta.get("shadow")) == bool(refine)) else None
        logger.info(f"Loaded existing collection: {self.collection_name} ({col.count()} rows)")

    def persist(self, first_new_row: Optional[int] = None, generation: bool = False):
        """Bring the files under persist_directory up to date.  With first_new_row = the files' row count, only rows
        [first_new_row, n) are APPENDED (create_index does this: O(batch)); otherwise everything is rewritten.
        generation=True (delete / update / upsert): everything is written as a NEW generation of files and the header switched
        to it last, so a crash leaves the previous state readable (see the comment above _persist_paths)."""
        if not self.persist_directory or self.collection is None:
            return
        import torch
        os.makedirs(self.persist_directory, exist_ok=True)
        col = self.collection
        generation = generation or self._gen_pending
        new_gen = (self._gen or 0) + 1 if generation else self._gen
        paths = self._persist_paths(new_gen)
        n = col.count()
        append = (not generation and first_new_row is not None and self._persisted_rows == first_new_row and first_new_row <= n)
        if generation:
            self._gen_pending = True        # until the header names the new files
            self._persisted_rows = None
        lo = first_new_row if append else 0
        pdim, dim = col.pdim, col.dim
        elem = 1 if col.slab_type == nat.SLAB_I8 else 2

        def new_rows(name):
            """rows [lo, n) of a per-shard array, in sidecar order"""
            parts, order = [], []
            for sh in col.shards:
                rg = sh.rows_global[: sh.n]
                sel = (rg >= lo).nonzero().flatten() if lo else None
                arr = getattr(sh, name)[: sh.n]
                parts.append((arr if sel is None else arr[sel]).cpu())
                order.append((rg if sel is None else rg[sel]).cpu())
            o = torch.cat(order).argsort()
            return torch.cat(parts)[o].contiguous().numpy()

        def write(key, arr, row_bytes):
            mode = "r+b" if (append and os.path.exists(paths[key])) else "wb"
            with open(paths[key], mode) as fh:
                if mode == "r+b":
                    fh.seek(lo * row_bytes)
                    fh.truncate()                 # drop anything a crashed add left past the header's row count
                fh.write(arr.tobytes())
                fh.flush()
                os.fsync(fh.fileno())

        write("slab", new_rows("slab"), pdim * elem)
        if col.slab_type == nat.SLAB_I8:
            write("scales", new_rows("scales"), 4)
        if col.refine_fp32:
            write("shadow", new_rows("shadow"), col.sdim * 4)
        elif not append and os.path.exists(paths["shadow"]):
            os.remove(paths["shadow"])
        # sidecar lines: keep the bytes the header vouches for (the first `lo` rows), replace the rest
        keep = self._docs_bytes if (append and os.path.exists(paths["docs"])) else 0
        with open(paths["docs"], "r+b" if keep else "wb") as fh:
            fh.seek(keep)
            fh.truncate()
            for r in range(lo if keep else 0, n):
                fh.write((json.dumps({"id": col.ids[r], "document": col.documents[r], "metadata": col.metadatas[r]}) + "\n").encode("utf-8"))
            fh.flush()
            os.fsync(fh.fileno())
            docs_bytes = fh.tell()
        if not generation:
            self._docs_bytes = docs_bytes
        meta = {"format": 2, "n": n, "dim": dim, "pdim": pdim, "index_dtype": col.index_dtype, "shadow": bool(col.refine_fp32),
                "row_err_max": max(sh.row_err_max() for sh in col.shards), "docs_bytes": docs_bytes}
        if col.space != nat.SPACE_COSINE:
            meta["space"], meta["norm_scale"] = self.space, col.shards[0].norm_scale_host
        if new_gen:
            meta["gen"] = int(new_gen)
        tmp = paths["meta"] + ".tmp"
        with open(tmp, "w") as fh:
            json.dump(meta, fh)
            fh.flush()
            os.fsync(fh.fileno())
        os.replace(tmp, paths["meta"])
        if generation:                                   # the header names the new files: they are the store now
            self._gen, self._docs_bytes, self._gen_pending = new_gen, docs_bytes, False
            self._remove_other_generations(new_gen)
        for key in ("legacy_slab", "legacy_docs"):       # superseded
            if os.path.exists(paths[key]):
                os.remove(paths[key])
        self._persisted_rows = n

    @staticmethod
    def _chunk_metadata(chunk, fields: Sequence[str]) -> dict:
        meta = {}
        for field in fields:
            value = getattr(chunk, field, None)
            if value is None:
                continue
            meta[field] = value if isinstance(value, (str, int, float)) else str(value)
        return meta

    # -- index build ---------------------------------------------------------------------------
    def create_index(self, chunks: List[Chunk], embeddings, metadata_fields: Optional[List[str]] = None):
        """Append chunks + their embeddings (numpy fp32 [n, d], or a cuda fp32 tensor) to the index."""
        if len(chunks) == 0:
            logger.warning("No chunks provided for indexing")
            return
        if len(chunks) != len(embeddings):
            raise ValueError(f"Chunk count ({len(chunks)}) doesn't match embedding count ({len(embeddings)})")
        fields = ['page_number', 'section', 'tokens'] if metadata_fields is None else metadata_fields
        try:
            import torch
            if self.collection is None:
                self.collection = self._new_collection()
                logger.info(f"Created new collection: {self.collection_name}")
            col = self.collection
            emb = self._as_f32(embeddings)
            if emb.ndim != 2:
                raise ValueError(f"embeddings must be 2-D, got shape {tuple(emb.shape)}")
            logger.info(f"Adding {len(chunks)} chunks to index...")
            start = len(col.ids)
            dist = self._dist()
            if col.space != nat.SPACE_COSINE:     # one device (__init__): the scale covers the batch before a row is written
                if col.dim is not None and emb.shape[1] != col.dim:
                    raise ValueError(f"Embedding dimension {emb.shape[1]} doesn't match the index dimension {col.dim}")
                emb = self._grow_scale(col.shards[0], emb)
            if dist is not None:      # SPMD: this rank keeps rows [lo, hi) of the batch on its GPU
                lo, hi = _shard.shard_slice(len(chunks), dist.get_world_size(), dist.get_rank())
                col.shards[0].append(emb[lo:hi].to(col.shards[0].device).contiguous(), start + lo)
            else:                     # one process: shard g of the batch goes to device g (one shard: everything)
                for sh, (lo, hi) in zip(col.shards, _shard.batch_slices(len(chunks), len(col.shards))):
                    sh.append(emb[lo:hi].to(sh.device).contiguous(), start + lo)
            if self.dedup_threshold is not None:
                # the device arrays hold the batch, the sidecars do not yet: drop its near-duplicates (of older rows, and of
                # earlier rows of the batch) BEFORE either sidecars or files see them -- one O(batch) append of the survivors
                dropped = set(self._drop_new_duplicates(start, len(chunks)).tolist())
                self.last_dedup = {"added": len(chunks) - len(dropped), "dropped": len(dropped)}
                if dropped:
                    logger.info(f"dedup_threshold {self.dedup_threshold}: dropped {len(dropped)} near-duplicate chunks of {len(chunks)}")
                    chunks = [c for at, c in enumerate(chunks) if at not in dropped]
            col.ids.extend(chunk.chunk_id for chunk in chunks)
            col.documents.extend(chunk.text for chunk in chunks)
            col.metadatas.extend(self._chunk_metadata(chunk, fields) for chunk in chunks)
            if self.persist_directory:
                self.persist(first_new_row=start)    # appends rows [start, n) when the files already hold [0, start)
            logger.info(f"Index created successfully! Total documents: {col.count()}")
        except (ValueError, nat.NativeError):
            raise
        except Exception as e:
            logger.error(f"Failed to add documents to collection: {e}")
            raise

    # -- one-document mutation (module docstring: delete / update / upsert) -------------------------------------
    @staticmethod
    def _as_f32(embeddings):
        import torch
        if isinstance(embeddings, torch.Tensor):
            return embeddings.to(dtype=torch.float32)
        return torch.from_numpy(np.ascontiguousarray(embeddings, dtype=np.float32))

    def _grow_scale(self, sh: _Shard, emb):
        """emb: fp32 [m, dim] anywhere -> the same rows, contiguous on the shard's device, after the shard's norm scale has been
        made to cover them: the batch's largest norm (crs::rows_norm_max: one launch, a 4-byte readback), ValueError before
        anything is written when it is not finite, and a rescale of the stored rows when the scale grows (which drops the filter
        cache, as an add does: the compacted sub-slabs hold rows under the old scale).  A cosine shard has no scale."""
        import torch
        emb = emb.to(sh.device).contiguous()
        if emb.shape[0] == 0 or sh.space == nat.SPACE_COSINE:
            return emb
        with torch.cuda.device(sh.device):
            top = nat.rows_norm_max(emb)
        if not np.isfinite(top):
            raise ValueError("an embedding has a non-finite norm; nothing was written")
        # R must cover the TRUE norms: the fp32 norm can fall short of them and round down onto a power of two (nat.covering_norm)
        if sh.grow_scale(nat.covering_norm(top, emb.shape[1])):
            self._filters = {}
            self._persisted_rows = None        # the files hold the rows under the old scale: the next persist rewrites them whole
        return emb

    def _mutated(self, ids_changed: bool, sidecars_changed: bool = True, documents_changed: bool = True):
        """Everything derived from rows dies: filter sub-slabs (keyed by row COUNT only: an update, or a delete followed by an
        equal add, would serve a stale one), the inverted metadata index, the id map (delete), the token CSR (a document changed),
        the SPMD wire blocks, the cached row error.  mutation_epoch tells the retriever's engine (graphs captured with the old row
        error) to rebuild."""
        self._filters = {}
        self._wire = {}
        if sidecars_changed or documents_changed or ids_changed:
            self.collection._drop_derived(ids_changed, metadata_changed=sidecars_changed, documents_changed=documents_changed)
        for sh in self.collection.shards:
            sh._row_err_host = None
        self.mutation_epoch += 1
        if self.persist_directory:
            self.persist(generation=True)

    @staticmethod
    def _local_rows(sh: _Shard, g_rows):
        """g_rows: ascending or arbitrary sidecar rows (int64 on the shard's device) -> (positions into g_rows of the rows this
        shard owns, their local rows).  rows_global is ascending on every layout (appends only ever add larger rows)."""
        import torch
        if sh.n == 0 or g_rows.numel() == 0:
            e = torch.zeros(0, dtype=torch.int64, device=sh.device)
            return e, e
        if sh.identity:
            sel = (g_rows < sh.n).nonzero().flatten()
            return sel, g_rows[sel]
        rg = sh.rows_global[: sh.n]
        pos = torch.searchsorted(rg, g_rows).clamp_(max=sh.n - 1)
        sel = (rg[pos] == g_rows).nonzero().flatten()
        return sel, pos[sel]

    def delete(self, ids: Optional[Sequence[str]] = None, where: Optional[dict] = None,
               where_document: Optional[dict] = None) -> int:
        """Remove the rows whose id is in `ids` AND that pass the filters (either part may be absent, not all three).  Unknown
        ids are ignored; an id that several rows carry removes all of them.  Returns the number of rows removed; 0 touches
        nothing.  The device arrays are compacted in place and in order (same capacity, same data_ptr): the store is then, row
        for row, what create_index of the survivors alone would have built, and searches return the same bits.  The tracked row
        error is left as it is (an upper bound stays an upper bound).  SPMD: the same call on every rank."""
        if ids is None and not where and not where_document:
            raise ValueError("delete needs ids, where or where_document")
        if self.collection is None:
            raise ValueError("No collection available. Create index first.")
        col = self.collection
        rows = None
        if ids is not None:
            idmap = col._id_rows()
            hit = [r for i in ([ids] if isinstance(ids, str) else ids) for r in idmap.get(i, ())]
            rows = np.unique(np.asarray(hit, dtype=np.int64))
        allowed = col.rows_matching(where, where_document)
        if allowed is not None:
            allowed = np.asarray(allowed, dtype=np.int64)
            rows = allowed if rows is None else np.intersect1d(rows, allowed)
        if rows.size == 0:
            return 0
        self._delete_rows(np.sort(rows))
        self._mutated(ids_changed=True)
        return int(rows.size)

    def _delete_rows(self, dead: np.ndarray):
        """dead: ascending distinct sidecar rows.  Every shard compacts the rows it owns (crs::slab_compact) and renumbers its
        row map; the host sidecars lose the same rows in one pass."""
        col = self.collection
        self._compact_shards(dead)
        keep = survivor_rows(len(col.ids), dead).tolist()
        col.ids = [col.ids[r] for r in keep]
        col.documents = [col.documents[r] for r in keep]
        col.metadatas = [col.metadatas[r] for r in keep]

    def _compact_shards(self, dead: np.ndarray):
        """The device half of _delete_rows: every shard drops the rows of `dead` (ascending distinct sidecar rows) it owns."""
        import torch
        col = self.collection
        for sh in col.shards:
            if sh.n == 0:
                continue
            with torch.cuda.device(sh.device):
                dead_t = torch.from_numpy(dead).to(sh.device)
                _, local = self._local_rows(sh, dead_t)
                m = int(local.numel())
                if m:
                    nat.slab_compact(local.contiguous(), sh.n, sh.slab, scales=sh.scales, shadow=sh.shadow,
                                     rows_global=None if sh.identity else sh.rows_global, first_row=int(local[0]))
                    # the kernel leaves the m rows past the survivors unspecified; a fresh store has zeros there
                    for arr in (sh.slab, sh.scales, sh.shadow):
                        if arr is not None:
                            arr[sh.n - m: sh.n].zero_()
                    sh.n -= m
                if not sh.identity and sh.n:
                    # new sidecar row = old - deleted sidecar rows below it (an identity shard's map is 0, 1, 2, ... before and after)
                    rg = sh.rows_global[: sh.n]
                    rg.sub_(torch.searchsorted(dead_t, rg))

    # -- near-duplicate detection (module docstring: near_duplicates / duplicate_of / deduplicate / dedup_threshold) ---------------
    def _join_refusals(self, threshold) -> float:
        """Everything that rules the join out, raised before any device work -> the threshold as a float."""
        if self.index_dtype == 'int8':
            raise NotImplementedError("near-duplicate detection is not supported with index_dtype 'int8': the int8 row error makes "
                                      "the candidate band wide, and the join needs an integer kernel of its own")
        if self.space != 'cosine':
            raise NotImplementedError(f"near-duplicate detection is not supported in space {self.space!r}: the threshold is a cosine")
        for layout, on in (("sharded=True", self.sharded), ("num_gpus > 1", self.num_gpus > 1), ("devices", bool(self._devices_cfg))):
            if on:
                raise NotImplementedError(f"near-duplicate detection is not supported with {layout}: a pair's rows would have to "
                                          "cross devices")
        if not self.refine_fp32:
            raise ValueError("near-duplicate detection needs the fp32 shadow (candidates are verified against it): refine_fp32 must "
                             "not be False")
        try:
            t = float(threshold)
        except (TypeError, ValueError):
            raise ValueError(f"threshold must be a number in (-1, 1], got {threshold!r}") from None
        if not (np.isfinite(t) and -1.0 < t <= 1.0):
            raise ValueError(f"threshold must be finite and in (-1, 1], got {threshold!r}")
        return t

    def _join(self, threshold: float, b_first: int, b_rows: int, max_pairs: int, n_rows: Optional[int] = None):
        """The two-stage join of the sole shard: every pair i < j, j in [b_first, b_first + b_rows), whose fp32 similarity is at
        least `threshold` -> (rows_a, rows_b int64, similarities fp32, sorted by (a, b); candidates; epsilon).  Stage 1
        (crs::pairs_above) runs over the slab at threshold - epsilon, stage 2 (crs::pairs_verify) over the fp32 shadow at the
        threshold.  The ranges are cut into stripes of _join_stripe_rows rows so that no launch exceeds the grid limit; a stripe
        whose candidates overflow its buffer is re-run once with a buffer of the reported size; more than max_pairs candidates in
        all raise ValueError naming the count.  One 8-byte readback per stripe launch."""
        import torch
        sh = self.collection.shards[0]
        n = sh.n if n_rows is None else int(n_rows)
        eps = nat.pairs_epsilon(sh.row_err_max(), sh.pdim)
        thr1, thr2 = nat.pairs_thresholds(threshold, eps)
        S = max(nat.PAIRS_TILE, int(self._join_stripe_rows) // nat.PAIRS_TILE * nat.PAIRS_TILE)
        out_a, out_b, out_s = [], [], []
        tally = {"stripes": 0, "reruns": 0, "candidates": 0}
        b_end = b_first + b_rows
        with torch.cuda.device(sh.device):
            for b0 in range(b_first, b_end, S):
                b1 = min(b0 + S, b_end)
                for a0 in range(0, b1 - 1, S):                       # i < j: rows at or past the stripe's last j pair with nothing
                    a1 = min(a0 + S, b1 - 1)
                    cap = max(0, min(int(self._join_first_cap), max_pairs - tally["candidates"]))
                    pairs, scores, count = nat.pairs_above(sh.slab, n, sh.dim, (a0, a1 - a0), (b0, b1 - b0), thr1, cap)
                    found = int(count.item())
                    tally["stripes"] += 1
                    if tally["candidates"] + found > max_pairs:
                        raise ValueError(f"near-duplicate join: at least {tally['candidates'] + found} candidate pairs at threshold "
                                         f"{threshold}, more than max_pairs = {max_pairs}; raise max_pairs or the threshold")
                    if found > cap:                                  # the stripe overflowed: once more, with room for all of it
                        tally["reruns"] += 1
                        pairs, scores, count = nat.pairs_above(sh.slab, n, sh.dim, (a0, a1 - a0), (b0, b1 - b0), thr1, found)
                        if int(count.item()) != found:
                            raise nat.NativeError("near-duplicate join: a stripe's candidate count changed between two runs")
                    tally["candidates"] += found
                    if found:
                        ra, rb, sims, kept = nat.pairs_verify(pairs[:found], sh.shadow, n, thr2)
                        k = int(kept.item())
                        out_a.append(ra[:k].cpu().numpy()); out_b.append(rb[:k].cpu().numpy()); out_s.append(sims[:k].cpu().numpy())
        self.last_join = tally
        a = np.concatenate(out_a) if out_a else np.zeros(0, dtype=np.int64)
        b = np.concatenate(out_b) if out_b else np.zeros(0, dtype=np.int64)
        s = np.concatenate(out_s) if out_s else np.zeros(0, dtype=np.float32)
        order = np.lexsort((b, a))
        return a[order], b[order], s[order], tally["candidates"], eps

    def _join_range(self, rows, n: int):
        if rows is None:
            return 0, n
        try:
            first, count = (int(v) for v in rows)
        except (TypeError, ValueError):
            raise ValueError(f"rows must be (first, count), got {rows!r}") from None
        if first < 0 or count < 0 or first + count > n:
            raise ValueError(f"rows = ({first}, {count}) leaves the collection's {n} rows")
        return first, count

    def near_duplicates(self, threshold: float, rows=None, max_pairs: int = 1 << 20) -> Dict[str, Any]:
        """Every pair of rows i < j whose cosine is at least `threshold`, each pair once (a thresholded self-join of the slab,
        csrc/join.hip).  GUARANTEE: the returned set is exactly {i < j : sim32(i, j) >= threshold}, sim32 being the verify
        kernel's fp32 dot of the two fp32 shadow rows (a fixed summation order); the fp16 stage runs at threshold - epsilon,
        epsilon = nat.pairs_epsilon(tracked row error, pdim), so it cannot miss a qualifying pair.
        rows=(first, count) restricts j to that range (i is any row below j): the incremental form, e.g. the new tail.
        Returns {'rows_a', 'rows_b' (int64, sidecar rows, sorted by (a, b)), 'similarities' (fp32), 'ids_a', 'ids_b',
        'candidates' (pairs the fp16 stage listed), 'epsilon'}.  More than max_pairs candidate pairs raise ValueError naming the
        count -- nothing is truncated silently.  fp16 cosine stores with the fp32 shadow on one device only."""
        t = self._join_refusals(threshold)
        if self.collection is None or self.collection.count() == 0:
            raise ValueError("No collection available. Create index first.")
        col = self.collection
        first, count = self._join_range(rows, col.count())
        a, b, s, cand, eps = self._join(t, first, count, int(max_pairs))
        return {"rows_a": a, "rows_b": b, "similarities": s, "ids_a": [col.ids[r] for r in a.tolist()],
                "ids_b": [col.ids[r] for r in b.tolist()], "candidates": cand, "epsilon": eps}

    def duplicate_of(self, threshold: float, rows=None) -> np.ndarray:
        """int64 [n]: -1 for a kept row, otherwise the kept row it duplicates -- greedy keep-first in row order over the pairs of
        near_duplicates(threshold, rows) (keep_first).  rows=(first, count): only rows of that range can be dropped."""
        found = self.near_duplicates(threshold, rows=rows, max_pairs=self.dedup_max_pairs)
        return keep_first(self.collection.count(), found["rows_a"], found["rows_b"])

    def deduplicate(self, threshold: float) -> int:
        """Remove every row duplicate_of(threshold) marks, through delete's path: the store is afterwards, row for row, what
        create_index of the survivors would have built.  Returns the number of rows removed."""
        dead = np.flatnonzero(self.duplicate_of(threshold) >= 0).astype(np.int64)
        if dead.size == 0:
            return 0
        self._delete_rows(dead)
        self._mutated(ids_changed=True)
        return int(dead.size)

    def _drop_new_duplicates(self, start: int, m: int) -> np.ndarray:
        """create_index with dedup_threshold: the shard already holds the m new rows [start, start + m), the sidecars do not.
        Joins all rows x the new tail, applies keep-first (old rows always kept), compacts the dropped rows out of the tail and
        returns their positions in the batch (ascending).  A failure takes the new rows off the shard again."""
        sh = self.collection.shards[0]
        try:
            a, b, _, _, _ = self._join(self._join_refusals(self.dedup_threshold), start, m, self.dedup_max_pairs, n_rows=start + m)
            dead = np.flatnonzero(keep_first(start + m, a, b) >= 0).astype(np.int64)
            if dead.size:
                self._compact_shards(dead)
            return dead - start
        except Exception:
            for arr in (sh.slab, sh.shadow):
                arr[start: start + m].zero_()
            sh.n = start
            raise

    def _plan_update(self, ids, embeddings, documents, metadatas):
        """Every check of update(), before anything changes -> (sidecar rows int64 [m], fp32 torch embeddings or None)."""
        if self.collection is None:
            raise ValueError("No collection available. Create index first.")
        col = self.collection
        ids = [ids] if isinstance(ids, str) else list(ids)
        for name, val in (("embeddings", embeddings), ("documents", documents), ("metadatas", metadatas)):
            if val is not None and len(val) != len(ids):
                raise ValueError(f"{name} count ({len(val)}) doesn't match id count ({len(ids)})")
        if len(set(ids)) != len(ids):
            raise ValueError("update: an id is given twice")
        idmap = col._id_rows()
        rows = []
        for i in ids:
            at = idmap.get(i)
            if not at:
                raise ValueError(f"update: unknown id {i!r}")
            if len(at) > 1:
                raise ValueError(f"update: id {i!r} is carried by {len(at)} rows")
            rows.append(at[0])
        emb = None
        if embeddings is not None:
            emb = self._as_f32(embeddings)
            if emb.ndim != 2:
                raise ValueError(f"embeddings must be 2-D, got shape {tuple(emb.shape)}")
            if len(ids) and emb.shape[1] != col.dim:
                raise ValueError(f"Embedding dimension {emb.shape[1]} doesn't match the index dimension {col.dim}")
        if metadatas is not None and not all(isinstance(m, dict) for m in metadatas):
            raise ValueError("metadatas must be dicts")
        return np.asarray(rows, dtype=np.int64), emb

    def _apply_update(self, rows: np.ndarray, emb, documents, metadatas):
        import torch
        col = self.collection
        if emb is not None:
            for sh in col.shards:
                if sh.n == 0:
                    continue
                with torch.cuda.device(sh.device):
                    sel, local = self._local_rows(sh, torch.from_numpy(rows).to(sh.device))
                    if sel.numel():
                        sh.store_rows(self._grow_scale(sh, emb.to(sh.device)[sel]), local.contiguous())
        for at, row in enumerate(rows.tolist()):
            if documents is not None:
                col.documents[row] = documents[at]
            if metadatas is not None:
                col.metadatas[row] = dict(metadatas[at])

    def update(self, ids: Sequence[str], embeddings=None, documents: Optional[Sequence[str]] = None,
               metadatas: Optional[Sequence[dict]] = None) -> None:
        """Per id, replace what is given: the embedding (the device rows are rewritten by the append's own per-row function),
        the document text, the metadata dict -- replaced WHOLE, not merged key by key (simpler than ChromaDB's update).
        An unknown id, an id that several rows carry, an id twice in one call, a length mismatch or a wrong dimension raise
        ValueError before anything is changed.  SPMD: the same call on every rank."""
        rows, emb = self._plan_update(ids, embeddings, documents, metadatas)
        if rows.size == 0 or (emb is None and documents is None and metadatas is None):
            return
        self._apply_update(rows, emb, documents, metadatas)
        self._mutated(ids_changed=False, sidecars_changed=metadatas is not None, documents_changed=documents is not None)

    def upsert(self, chunks: List[Chunk], embeddings, metadata_fields: Optional[List[str]] = None) -> None:
        """create_index's signature: chunks whose chunk_id exists are updated in place (embedding, text, metadata), the others
        are appended in their given order by create_index."""
        if len(chunks) != len(embeddings):
            raise ValueError(f"Chunk count ({len(chunks)}) doesn't match embedding count ({len(embeddings)})")
        if len(chunks) == 0:
            return
        if self.collection is None or self.collection.count() == 0:
            self.create_index(chunks, embeddings, metadata_fields)
            self.mutation_epoch += 1
            return
        col = self.collection
        fields = ['page_number', 'section', 'tokens'] if metadata_fields is None else metadata_fields
        emb = self._as_f32(embeddings)
        if emb.ndim != 2:
            raise ValueError(f"embeddings must be 2-D, got shape {tuple(emb.shape)}")
        if emb.shape[1] != col.dim:
            raise ValueError(f"Embedding dimension {emb.shape[1]} doesn't match the index dimension {col.dim}")
        idmap = col._id_rows()
        known = [a for a, c in enumerate(chunks) if c.chunk_id in idmap]
        fresh = [a for a, c in enumerate(chunks) if c.chunk_id not in idmap]
        rows, emb_known = self._plan_update([chunks[a].chunk_id for a in known], emb[known] if known else None,
                                            [chunks[a].text for a in known] if known else None,
                                            [self._chunk_metadata(chunks[a], fields) for a in known] if known else None)
        if known:
            self._apply_update(rows, emb_known, [chunks[a].text for a in known],
                               [self._chunk_metadata(chunks[a], fields) for a in known])
            self._mutated(ids_changed=False)
        else:
            self.mutation_epoch += 1
        if fresh:
            self.create_index([chunks[a] for a in fresh], emb[fresh], metadata_fields)

    # -- search --------------------------------------------------------------------------------
    def _cap(self, top_k: int) -> int:
        return _search.first_cap(self.exact_cap, top_k)

    _order = staticmethod(_search.order)

    def _filtered_view(self, g: int, sh: _Shard, filt: dict) -> _search.ShardView:
        """The allowed rows shard g owns, compacted ONCE per distinct filter into a sub-slab (+ scales, shadow, row map) and
        kept with the filter's cache entry: a filtered query then costs one scan of exactly the allowed rows -- no per-query
        gather, no Python pass over the metadata (the reference hands `where` to ChromaDB, rag/indexing.py:129-130,174)."""
        import dataclasses
        import torch
        sub = filt["shards"].get(g)
        if sub is None:
            allowed_t = torch.as_tensor(filt["rows"], dtype=torch.int64, device=sh.device)
            if sh.identity:
                local = allowed_t[allowed_t < sh.n]
            else:
                local = torch.isin(sh.rows_global[:sh.n], allowed_t).nonzero().flatten()
            pick = lambda arr: None if arr is None else arr[local].contiguous()                # noqa: E731
            sub = filt["shards"][g] = dataclasses.replace(sh.view(), slab=pick(sh.slab), scales=pick(sh.scales), shadow=pick(sh.shadow),
                                                          n=int(local.numel()), row_map=pick(sh.rows_global))
        return sub

    def _search_shard(self, g: int, q32, top_k: int, filt, cap: int):
        """q32: fp32 [nq, dim] on any device -> (scores [nq, top_k], GLOBAL sidecar rows [nq, top_k], certificate status int32
        [nq] or None) on shard g's device, from its rows or (metadata filter) the cached, compacted sub-slab of the allowed rows it
        owns.  Nothing here waits for the device."""
        import torch
        sh = self.collection.shards[g]
        with torch.cuda.device(sh.device):
            q = q32 if q32.device == sh.device else q32.to(sh.device, non_blocking=True)
            view = sh.view() if (filt is None or sh.n == 0) else self._filtered_view(g, sh, filt)
            return _search.search_view(view, q, top_k, self.refine_overfetch, cap, _search.escalates(self.refine_exact, sh.slab_type))

    def _topk_device(self, q32, top_k: int, filt=None):
        """q32: fp32 [nq, dim] on the first device -> (scores [nq, k] fp32, sidecar rows [nq, k] int64) there and the exactness
        tally of THIS search, whatever its path (see __init__).  filt: a filter cache entry (_filter_entry) or None."""
        import torch
        col = self.collection
        nq = q32.shape[0]
        cap = self._cap(top_k)
        # launches are asynchronous: the devices scan their shards concurrently; then, shard by shard, the one host wait of a
        # refined search (search_batch reads the results right after anyway) and the repeats with a longer escalation list
        parts = [self._search_shard(g, q32, top_k, filt, cap) for g in range(len(col.shards))]
        parts = [_search.resolve_overflow(part, lambda c, g=g: self._search_shard(g, q32, top_k, filt, c), cap, top_k)
                 for g, part in enumerate(parts)]
        tally = _search.tally([st for _, _, st in parts], nq, top_k, col.refine_fp32,
                              _search.escalates(self.refine_exact, col.slab_type))
        if len(parts) > 1:             # one process, N devices: partial lists to the first device, merge there
            dev0 = col.device
            with torch.cuda.device(dev0):
                s, i = _search.merge_lists(torch.stack([s.to(dev0) for s, _, _ in parts]).contiguous(),
                                           torch.stack([i.to(dev0) for _, i, _ in parts]).contiguous(), top_k)
        else:
            s, i, _ = parts[0]
        dist = self._dist()
        if dist is not None:           # SPMD: ONE all-gather of the wire blocks, k-way merge on every rank
            if top_k > nat.MAX_K_CERT:
                raise ValueError(f"top_k {top_k} > {nat.MAX_K_CERT} is not supported on an SPMD-sharded store")
            key = (nq, top_k, dist.get_world_size())
            wb = self._wire.get(key)
            if wb is None:
                wb = self._wire[key] = nat.WireBlock(nq, top_k, col.device, dist.get_world_size())
            wb.scores.copy_(s)
            wb.ids.copy_(i)
            # above MAX_K the shards' lists (certified, escalated or the GEMM path's) arrive sorted: the co-ranking merge
            s, i = _shard.allgather_merge(dist, wb.buf, wb.gathered, nq, top_k, top_k,
                                          nat.merge_topk_wire if top_k <= nat.MAX_K else nat.merge_sorted_wire)
        return s, i, tally

    def _filter_entry(self, where: Optional[dict], where_document: Optional[dict]):
        """Cache entry of a distinct (where, where_document) pair: the allowed sidecar rows (SlabCollection.rows_matching:
        an inverted metadata index, no per-query pass over the rows) and, filled by the first search, each shard's compacted
        sub-slab.  None = no filter.  Entries die when rows are added; the eight most recent filters are kept."""
        if not where and not where_document:
            return None
        col = self.collection
        try:
            key = json.dumps([where, where_document], sort_keys=True, default=repr)
        except TypeError:
            key = repr((where, where_document))
        ent = self._filters.get(key)
        if ent is None or ent["n"] != col.count():
            ent = {"n": col.count(), "rows": col.rows_matching(where, where_document), "shards": {}}
            self._filters.pop(key, None)
            while len(self._filters) >= 8:
                self._filters.pop(next(iter(self._filters)))
            self._filters[key] = ent
        return ent

    def search(self, query_embedding, top_k: int = 5, where: Optional[dict] = None,
               where_document: Optional[dict] = None) -> Dict[str, Any]:
        """Nearest chunks for ONE query.  Returns {'ids','documents','metadatas','distances'} as
        lists of one list each; distances are cosine distances (1 - cos), ascending (space 'ip': 1 - <q, x>, 'l2': the squared
        Euclidean distance -- ChromaDB's, computed in fp32 from the caller's vectors; equal distances: lower row first)."""
        if self.collection is None:
            raise ValueError("No collection available. Create index first.")
        if self.collection.count() == 0:
            logger.warning("Collection is empty. No results to return.")
            return {k: [[]] for k in _EMPTY}
        top_k = min(top_k, self.collection.count())
        # the reference flattens whatever it is given into one vector (indexing.py:156-168)
        if isinstance(query_embedding, np.ndarray):
            flat = query_embedding.reshape(-1)
        else:
            flat = np.asarray(list(query_embedding), dtype=np.float32).reshape(-1)
        try:
            res = self.search_batch(flat.reshape(1, -1), top_k, where=where, where_document=where_document)
            return {key: [res[key][0]] for key in ('ids', 'documents', 'metadatas', 'distances')}
        except Exception as e:
            logger.error(f"Search failed: {e}")
            raise

    def _sole_shard(self, fp32: bool = False):
        """The one shard of a store whose local rows ARE the sidecar rows (fp32: and that keeps the fp32 rows), or None."""
        col = self.collection
        if col is None or len(col.shards) != 1 or not col.shards[0].identity or (fp32 and col.shards[0].shadow is None):
            return None
        return col.shards[0]

    def engine_view(self):
        """This store as ONE device shard for rag._engine.RetrievalEngine, or None when its layout needs the general path
        (several devices, SPMD sharding, a non-identity row map)."""
        sh = self._sole_shard()
        if sh is None or self.sharded or sh.n == 0 or sh.space != nat.SPACE_COSINE:   # the engine's graphs convert queries for cosine
            return None
        return sh.view()

    def rows_f32(self, rows):
        """The fp32 rows the store kept for these sidecar rows (numpy [len(rows), dim]; the normalised encoder output of the
        chunks as indexed), or None when it keeps none / the layout is not a single identity shard.  Space 'ip' / 'l2': the
        caller's own vectors x, recovered exactly from the stored rows (x = R u, x = 2R v: a power of two)."""
        import torch
        sh = self._sole_shard(fp32=True)
        if sh is None:
            return None
        idx = torch.as_tensor(np.asarray(rows, dtype=np.int64), device=sh.device)
        if sh.space == nat.SPACE_COSINE:
            return sh.shadow[idx].cpu().numpy()
        back = sh.norm_scale_host * (2.0 if sh.space == nat.SPACE_L2 else 1.0)
        return (sh.shadow[idx, :sh.dim] * back).cpu().numpy()

    def attach_token_encoder(self, reranker) -> None:
        """The LateInteractionReranker (rag/late_interaction.py) whose token vectors token_index() holds.  Attaching another one
        forgets the index built with the previous one."""
        self._token_encoder = reranker

    def token_index(self, reranker=None) -> _TokenIndex:
        """The late-interaction token index of the collection (_TokenIndex: tok16, n_tokens, offsets, offsets_dev, n_rows) for the
        attached encoder (`reranker`, when given, is attached first).  Built on first use; afterwards only the rows that arrived
        since are encoded.  A delete, a document update or an upsert drops it (SlabCollection._drop_derived) and the next call
        re-encodes every document.  Not persisted; one device only.  ValueError when it would exceed max_index_bytes."""
        import torch
        if reranker is not None and reranker is not self._token_encoder:
            self.attach_token_encoder(reranker)
        if self._token_encoder is None:
            raise ValueError("no token encoder attached: call attach_token_encoder(LateInteractionReranker(...)) first")
        col = self.collection
        if col is None:
            raise ValueError("No collection available. Create index first.")
        if self.sharded or len(col.shards) != 1:
            raise NotImplementedError("the late-interaction token index lives on one device: sharded / num_gpus / devices are not supported")
        limit = self.max_index_bytes
        if limit is None:
            limit = torch.cuda.get_device_properties(col.device).total_memory // 2
        return col._token_index(self._token_encoder, int(limit))

    def attach_sparse_encoder(self, encoder) -> None:
        """The SparseEncoder (rag/sparse.py) whose document vectors sparse_index() holds and whose queries sparse_rows() encodes.
        Attaching another one forgets the index built with the previous one."""
        self._sparse_encoder = encoder

    def sparse_index(self, encoder=None) -> _SparseIndex:
        """The learned-sparse index of the collection (_SparseIndex: tokens, weights, n_terms, offsets, offsets_dev, n_rows) for the
        attached encoder (`encoder`, when given, is attached first).  Built on first use; afterwards only the rows that arrived
        since are encoded.  A delete, a document update or an upsert drops it (SlabCollection._drop_derived) and the next call
        re-encodes every document.  Not persisted; one device only.  ValueError, before any encoding, when rows x sparse_doc_terms
        x 8 bytes would exceed max_index_bytes."""
        import torch
        if encoder is not None and encoder is not self._sparse_encoder:
            self.attach_sparse_encoder(encoder)
        if self._sparse_encoder is None:
            raise ValueError("no sparse encoder attached: call attach_sparse_encoder(SparseEncoder(...)) first")
        col = self.collection
        if col is None:
            raise ValueError("No collection available. Create index first.")
        if self.sharded or len(col.shards) != 1:
            raise NotImplementedError("the sparse index lives on one device: sharded / num_gpus / devices are not supported")
        limit = self.max_index_bytes
        if limit is None:
            limit = torch.cuda.get_device_properties(col.device).total_memory // 2
        return col._sparse_index(self._sparse_encoder, self.sparse_doc_terms, int(limit))

    def sparse_rows(self, queries: Sequence[str], top_k: int):
        """Exact learned-sparse top-k of every query over the WHOLE collection, on the device (crs_sparse_topk,
        csrc/sparse_scan.hip): queries [nq] strings -> (scores fp32 [nq, top_k], sidecar rows int64 [nq, top_k]) as numpy, best
        first, ties by lower row, (-inf, -1) past the hits (a row that shares no term with the query is no hit).  The queries are
        encoded on the device to at most sparse_query_terms terms each and go to the scan as they are: a query's padded slots
        (-1, 0) are pairs no row matches, so nothing comes back to the host in between.  The batch is cut as bm25_rows cuts it
        (_bm25_launches: 64 queries, BM25_MAX_PAIRS pairs, every query counting sparse_query_terms); one readback for the whole
        call.  1 <= top_k <= MAX_K."""
        import torch
        if not isinstance(top_k, (int, np.integer)) or isinstance(top_k, bool) or not 1 <= top_k <= nat.MAX_K:
            raise ValueError(f"top_k must be an integer in 1..{nat.MAX_K} for a sparse search, got {top_k!r}")
        index = self.sparse_index()
        queries = list(queries)
        nq, k, cap = len(queries), int(top_k), self.sparse_query_terms
        scores = np.full((nq, k), -np.inf, dtype=np.float32)
        rows = np.full((nq, k), -1, dtype=np.int64)
        self.last_sparse = {'queries': nq, 'query_terms': cap, 'launches': 0}
        if nq == 0 or index.n_rows == 0:
            return scores, rows
        launches = self._bm25_launches([cap] * nq)
        dev = index.device
        with self._device_guard(dev):
            q_ids, q_w, _ = self._sparse_encoder.encode_queries_device(queries, cap)
            out = torch.empty(nq * k + (nq * k + 1) // 2, dtype=torch.int64, device=dev)
            out_r = out[: nq * k].view(nq, k)
            out_s = out[nq * k:].view(torch.float32)[: nq * k].view(nq, k)
            q_off = torch.arange(0, (nat.BM25_MAX_QUERIES + 1) * cap, cap, dtype=torch.int64, device=dev)
            for lo, hi in launches:
                n = hi - lo
                nat.sparse_topk(index.offsets_dev, index.tokens, index.weights, index.n_rows, q_off[: n + 1],
                                q_ids[lo:hi].reshape(-1), q_w[lo:hi].reshape(-1), k, out_scores=out_s[lo:hi], out_rows=out_r[lo:hi])
            host = out.cpu().numpy()
        self.last_sparse['launches'] = len(launches)
        rows[:] = host[: nq * k].reshape(nq, k)
        scores[:] = host[nq * k:].view(np.float32)[: nq * k].reshape(nq, k)
        return scores, rows

    def search_sparse_batch(self, queries: Sequence[str], top_k: int = 5) -> Dict[str, Any]:
        """search_lexical_batch for the learned-sparse list (sparse_rows): the same dict, 'scores' the sparse dot products."""
        return self._rows_dict(*self.sparse_rows(queries, top_k))

    def mmr_order(self, rows, rel, counts, lam: float):
        """Greedy MMR order of many result lists at once, on the device (crs_mmr_order, csrc/mmr.hip): rows int64 / rel fp64
        [nq, m_max <= MAX_K] (sidecar rows and their relevance, list order), counts [nq], lam = 1 - diversity_penalty -> numpy
        int32 [nq, m_max], the first counts[i] slots the positions of list i in MMR order, the others -1.  One upload of the
        three arrays, one launch over the fp32 rows in place, one readback.  None when the store cannot serve it (the
        conditions of rows_f32: no fp32 rows kept, or not a single identity shard) or a list is longer than MAX_K."""
        import torch
        sh = self._sole_shard(fp32=True)
        if sh is None or sh.space != nat.SPACE_COSINE:      # the kernel reads the shadow as unit rows of `dim` coordinates
            return None
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        if rows.ndim != 2 or not 1 <= rows.shape[1] <= nat.MAX_K:
            return None
        nq, m_max = rows.shape
        # one host block -> one copy: [rows int64 | rel fp64 | counts int32 (padded to 8 bytes)]
        block = np.empty(2 * nq * m_max + (nq + 1) // 2, dtype=np.int64)
        block[:nq * m_max] = rows.ravel()
        block[nq * m_max:2 * nq * m_max].view(np.float64)[:] = np.asarray(rel, dtype=np.float64).ravel()
        block[2 * nq * m_max:].view(np.int32)[:nq] = np.asarray(counts, dtype=np.int32)
        dev = torch.from_numpy(block).to(sh.device)
        with torch.cuda.device(sh.device):
            order = nat.mmr_order(sh.shadow, sh.n, dev[:nq * m_max].view(nq, m_max),
                                  dev[nq * m_max:2 * nq * m_max].view(torch.float64).view(nq, m_max),
                                  dev[2 * nq * m_max:].view(torch.int32)[:nq], float(lam))
        return order.cpu().numpy()

    def rerank_lexical(self, queries: Sequence[str], scores, rows, k: int, threshold: float):
        """The post-search steps of ContextRetriever.retrieve_batch for many result lists at once, on the device
        (crs_rerank_lexical, csrc/rerank.hip): queries [nq] strings, scores fp32 / rows int64 [nq, m_max <= MAX_K] (the store's
        cosine scores and sidecar rows in list order, -1 rows = empty slots), k the list length wanted, threshold the
        similarity_threshold -> numpy (order int32 [nq, m_max]: input positions, -1 past the count; count int32 [nq]; sim fp64
        [nq, m_max] by input position; rr fp64 [nq, m_max]: the re-rank score where reranked; reranked int32 [nq]), in the bits of
        the host rule.  The queries are tokenised against the collection's vocabulary (SlabCollection._token_csr); one host block
        up, one launch, one block back.  Works on every layout (the rows are sidecar rows).  None when a list is longer than
        MAX_K or the native library was built without the kernel."""
        import torch
        col = self.collection
        if col is None:
            raise ValueError("No collection available. Create index first.")
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        scores = np.ascontiguousarray(scores, dtype=np.float32)
        if rows.ndim != 2 or scores.shape != rows.shape or not 1 <= rows.shape[1] <= nat.MAX_K or not nat.has_rerank_lexical():
            return None
        nq, m_max = rows.shape
        if len(queries) != nq:
            raise ValueError(f"Query count ({len(queries)}) doesn't match list count ({nq})")
        if nq == 0:
            return (np.zeros((0, m_max), np.int32), np.zeros(0, np.int32), np.zeros((0, m_max)), np.zeros((0, m_max)), np.zeros(0, np.int32))
        csr = col._token_csr()
        q_ids, q_norm = zip(*(csr.query_ids(q) for q in queries))
        q_off = np.zeros(nq + 1, dtype=np.int64)
        np.cumsum([len(ids) for ids in q_ids], out=q_off[1:])
        n_tok, cells = int(q_off[-1]), nq * m_max
        # one host block -> one copy: [rows int64 | q_offsets int64 | scores fp32 | q_norm int32 | q_tokens int32], int64 words
        w_sc, w_norm, w_tok = (cells + 1) // 2, (nq + 1) // 2, (n_tok + 1) // 2
        o_off = cells
        o_sc = o_off + nq + 1
        o_norm = o_sc + w_sc
        o_tok = o_norm + w_norm
        block = np.zeros(o_tok + w_tok, dtype=np.int64)
        block[:cells] = rows.ravel()
        block[o_off:o_sc] = q_off
        block[o_sc:o_norm].view(np.float32)[:cells] = scores.ravel()
        block[o_norm:o_tok].view(np.int32)[:nq] = q_norm
        block[o_tok:].view(np.int32)[:n_tok] = np.fromiter((t for ids in q_ids for t in ids), dtype=np.int32, count=n_tok)
        dev = col.device
        with torch.cuda.device(dev):
            doc_off, doc_tok = csr.device(dev)
            d = torch.from_numpy(block).to(dev)
            # one device block <- the five outputs: [sim fp64 | rr fp64 | order int32 | count int32 | reranked int32]
            w_ord, w_cnt = (cells + 1) // 2, (nq + 1) // 2
            out = torch.empty(2 * cells + w_ord + 2 * w_cnt, dtype=torch.int64, device=dev)
            sim_d = out[:cells].view(torch.float64).view(nq, m_max)
            rr_d = out[cells:2 * cells].view(torch.float64).view(nq, m_max)
            ord_d = out[2 * cells:2 * cells + w_ord].view(torch.int32)[:cells].view(nq, m_max)
            cnt_d = out[2 * cells + w_ord:2 * cells + w_ord + w_cnt].view(torch.int32)[:nq]
            rer_d = out[2 * cells + w_ord + w_cnt:].view(torch.int32)[:nq]
            nat.rerank_lexical(d[o_sc:o_norm].view(torch.float32)[:cells].view(nq, m_max), d[:cells].view(nq, m_max), doc_off, doc_tok,
                               len(col.documents), d[o_off:o_sc], d[o_tok:].view(torch.int32)[:n_tok], d[o_norm:o_tok].view(torch.int32)[:nq],
                               int(k), float(threshold), out=(ord_d, cnt_d, sim_d, rr_d, rer_d))
            host = out.cpu().numpy()
        return (host[2 * cells:2 * cells + w_ord].view(np.int32)[:cells].reshape(nq, m_max),
                host[2 * cells + w_ord:2 * cells + w_ord + w_cnt].view(np.int32)[:nq],
                host[:cells].view(np.float64).reshape(nq, m_max), host[cells:2 * cells].view(np.float64).reshape(nq, m_max),
                host[2 * cells + w_ord + w_cnt:].view(np.int32)[:nq])

    # -- hybrid retrieval: the lexical list (csrc/bm25.hip) and the fusion of the two lists (csrc/fuse.hip) -------------------------
    @staticmethod
    def _device_guard(dev):
        """torch.cuda.device(dev) for a HIP device, nothing for any other (the host-side tests run the callers of the native
        wrappers with those wrappers replaced, on CPU tensors)."""
        import contextlib
        import torch
        return torch.cuda.device(dev) if torch.device(dev).type == "cuda" else contextlib.nullcontext()

    @staticmethod
    def bm25_constants(n_rows: int, total_len: int, k1: float, b: float):
        """(c0, c1, k1 + 1) of crs_bm25_topk, each computed in fp64 and rounded once to fp32: dn = c0 + c1 * len with
        c0 = k1 (1 - b), c1 = k1 b / avgdl, avgdl = total_len / n_rows (c1 = 0 when every document is empty)."""
        k1, b = float(k1), float(b)
        c1 = k1 * b / (total_len / n_rows) if total_len > 0 and n_rows > 0 else 0.0
        return np.float32(k1 * (1.0 - b)), np.float32(c1), np.float32(k1 + 1.0)

    @staticmethod
    def bm25_weight(n_rows: int, df: int) -> np.float32:
        """w_t = ln(1 + (N - df + 0.5) / (df + 0.5)) in fp64 (Lucene's non-negative idf), rounded once to fp32."""
        import math
        return np.float32(math.log(1.0 + (n_rows - df + 0.5) / (df + 0.5)))

    @staticmethod
    def _bm25_launches(lengths: Sequence[int]):
        """Cut a query batch into launches: consecutive (lo, hi) ranges of at most BM25_MAX_QUERIES queries and BM25_MAX_PAIRS
        (query, known token) pairs.  A single query above the pair cap cannot be served: ValueError."""
        out, lo, pairs = [], 0, 0
        for i, n in enumerate(lengths):
            if n > nat.BM25_MAX_PAIRS:
                raise ValueError(f"query {i} has {n} distinct known tokens; one BM25 launch takes at most {nat.BM25_MAX_PAIRS}")
            if i - lo == nat.BM25_MAX_QUERIES or pairs + n > nat.BM25_MAX_PAIRS:
                out.append((lo, i))
                lo, pairs = i, 0
            pairs += n
        if lo < len(lengths):
            out.append((lo, len(lengths)))
        return out

    def bm25_rows(self, queries: Sequence[str], top_k: int, k1: float = 1.5, b: float = 0.75):
        """Exact Okapi BM25 top-k of every query over the WHOLE collection, on the device (crs_bm25_topk, csrc/bm25.hip): queries
        [nq] strings -> (scores fp32 [nq, top_k], sidecar rows int64 [nq, top_k]) as numpy, best first, ties by lower row, (-inf, -1)
        past the hits (a row that shares no token with the query is no hit).  The queries are tokenised against the collection's
        vocabulary (SlabCollection._token_csr: lower().split(), the retriever's own rule); idf weights, N, df and avgdl are taken
        over the whole collection and computed in fp64; the kernel's fp32 arithmetic is a pure function of its inputs
        (include/crs_hip.h).  The batch is cut at 64 queries and at BM25_MAX_PAIRS (query, token) pairs per launch; one host
        block up per launch, one readback for the whole call.  Runs on the first device over the sidecar rows, so it serves
        every layout.  1 <= top_k <= MAX_K."""
        import torch
        col = self.collection
        if col is None:
            raise ValueError("No collection available. Create index first.")
        if not isinstance(top_k, (int, np.integer)) or isinstance(top_k, bool) or not 1 <= top_k <= nat.MAX_K:
            raise ValueError(f"top_k must be an integer in 1..{nat.MAX_K} for a lexical search, got {top_k!r}")
        if not (k1 >= 0 and np.isfinite(k1)) or not 0.0 <= b <= 1.0:
            raise ValueError(f"BM25 needs a finite k1 >= 0 and 0 <= b <= 1, got k1={k1!r}, b={b!r}")
        queries = list(queries)
        nq, k = len(queries), int(top_k)
        scores = np.full((nq, k), -np.inf, dtype=np.float32)
        rows = np.full((nq, k), -1, dtype=np.int64)
        csr = col._token_csr()
        n_rows = csr.rows
        if nq == 0 or n_rows == 0:
            return scores, rows
        q_ids = [csr.query_ids(q)[0] for q in queries]
        launches = self._bm25_launches([len(ids) for ids in q_ids])
        c0, c1, k1p1 = self.bm25_constants(n_rows, csr.total_len, k1, b)
        df = csr.df
        dev = col.device
        with self._device_guard(dev):
            doc_off, doc_tok = csr.device(dev)
            doc_tf, doc_len = csr.device_stats(dev)
            # one device block <- both outputs of every launch: [rows int64 [nq, k] | scores fp32 [nq, k]]
            out = torch.empty(nq * k + (nq * k + 1) // 2, dtype=torch.int64, device=dev)
            out_r = out[: nq * k].view(nq, k)
            out_s = out[nq * k:].view(torch.float32)[: nq * k].view(nq, k)
            for lo, hi in launches:
                n, ids = hi - lo, q_ids[lo:hi]
                n_tok = sum(len(t) for t in ids)
                # one host block -> one copy: [q_offsets int64 [n + 1] | q_tokens int32 | q_weights fp32], int64 words
                w_tok = (n_tok + 1) // 2
                block = np.zeros(n + 1 + 2 * w_tok, dtype=np.int64)
                np.cumsum([len(t) for t in ids], out=block[1:n + 1])
                flat = np.fromiter((t for ts in ids for t in ts), dtype=np.int32, count=n_tok)
                block[n + 1:n + 1 + w_tok].view(np.int32)[:n_tok] = flat
                block[n + 1 + w_tok:].view(np.float32)[:n_tok] = [self.bm25_weight(n_rows, int(df[t])) for t in flat.tolist()]
                d = torch.from_numpy(block).to(dev)
                nat.bm25_topk(doc_off, doc_tok, doc_tf, doc_len, n_rows, d[: n + 1], d[n + 1:n + 1 + w_tok].view(torch.int32)[:n_tok],
                              d[n + 1 + w_tok:].view(torch.float32)[:n_tok], float(c0), float(c1), float(k1p1), k,
                              out_scores=out_s[lo:hi], out_rows=out_r[lo:hi])
            host = out.cpu().numpy()
        rows[:] = host[: nq * k].reshape(nq, k)
        scores[:] = host[nq * k:].view(np.float32)[: nq * k].reshape(nq, k)
        return scores, rows

    def search_lexical_batch(self, queries: Sequence[str], top_k: int = 5) -> Dict[str, Any]:
        """search_batch for the lexical list (bm25_rows): the same dict with 'scores' (BM25, best first) in place of 'distances'."""
        return self._rows_dict(*self.bm25_rows(queries, top_k))

    def _rows_dict(self, sc, rh) -> Dict[str, Any]:
        col = self.collection
        out = {'ids': [], 'documents': [], 'metadatas': [], 'scores': []}
        for a in range(len(rh)):
            valid = [r for r in rh[a].tolist() if r >= 0]
            out['ids'].append([col.ids[r] for r in valid])
            out['documents'].append([col.documents[r] for r in valid])
            out['metadatas'].append([col.metadatas[r] for r in valid])
            out['scores'].append(sc[a, : len(valid)].astype(np.float64).tolist())
        return out

    def fuse_rrf(self, dense_rows, lex_rows, k_out: int, c: float = 60.0, weights=(1.0, 1.0)):
        """Weighted reciprocal rank fusion of a dense and a lexical list per query, on the device (crs_fuse_rrf, csrc/fuse.hip):
        dense_rows int64 [nq, m_dense <= MAX_K], lex_rows int64 [nq, m_lex <= MAX_K] (sidecar rows in rank order, -1 = empty slot)
        -> numpy (rows int64, fused fp64, dense_pos int32, lex_pos int32, each [nq, k_out]; count int32 [nq]): fused =
        weights[0] / (c + i + 1) + weights[1] / (c + j + 1) for a row at 0-based positions i and j (a row in one list only: that
        term alone), ordered by fused descending, then dense position, then lexical position; past the count (-1, 0, -1, -1).
        One block up, one launch, one block back."""
        import torch
        col = self.collection
        if col is None:
            raise ValueError("No collection available. Create index first.")
        dense_rows = np.ascontiguousarray(dense_rows, dtype=np.int64)
        lex_rows = np.ascontiguousarray(lex_rows, dtype=np.int64)
        if dense_rows.ndim != 2 or lex_rows.ndim != 2 or dense_rows.shape[0] != lex_rows.shape[0]:
            raise ValueError("dense_rows and lex_rows must be [nq, m_dense] and [nq, m_lex]")
        if not (1 <= dense_rows.shape[1] <= nat.MAX_K and 1 <= lex_rows.shape[1] <= nat.MAX_K and 1 <= int(k_out) <= 2 * nat.MAX_K):
            raise ValueError(f"fuse_rrf takes lists of 1..{nat.MAX_K} rows and 1 <= k_out <= {2 * nat.MAX_K}")
        w_d, w_l = (float(w) for w in weights)
        nq, k_out = dense_rows.shape[0], int(k_out)
        cells, w_pos, w_cnt = nq * k_out, (nq * k_out + 1) // 2, (nq + 1) // 2
        if nq == 0:
            return (np.zeros((0, k_out), np.int64), np.zeros((0, k_out)), np.zeros((0, k_out), np.int32), np.zeros((0, k_out), np.int32),
                    np.zeros(0, np.int32))
        dev = col.device
        with self._device_guard(dev):
            d = torch.from_numpy(np.concatenate([dense_rows.ravel(), lex_rows.ravel()])).to(dev)
            # one device block <- the five outputs: [rows int64 | fused fp64 | dense_pos int32 | lex_pos int32 | count int32]
            out = torch.empty(2 * cells + 2 * w_pos + w_cnt, dtype=torch.int64, device=dev)
            tens = (out[:cells].view(nq, k_out), out[cells:2 * cells].view(torch.float64).view(nq, k_out),
                    out[2 * cells:2 * cells + w_pos].view(torch.int32)[:cells].view(nq, k_out),
                    out[2 * cells + w_pos:2 * cells + 2 * w_pos].view(torch.int32)[:cells].view(nq, k_out),
                    out[2 * cells + 2 * w_pos:].view(torch.int32)[:nq])
            nat.fuse_rrf(d[: dense_rows.size].view(dense_rows.shape), d[dense_rows.size:].view(lex_rows.shape), k_out, float(c), w_d, w_l,
                         out=tens)
            host = out.cpu().numpy()
        return (host[:cells].reshape(nq, k_out), host[cells:2 * cells].view(np.float64).reshape(nq, k_out),
                host[2 * cells:2 * cells + w_pos].view(np.int32)[:cells].reshape(nq, k_out),
                host[2 * cells + w_pos:2 * cells + 2 * w_pos].view(np.int32)[:cells].reshape(nq, k_out),
                host[2 * cells + 2 * w_pos:].view(np.int32)[:nq])

    def _search_rows(self, query_embeddings, top_k: int, where: Optional[dict] = None, where_document: Optional[dict] = None):
        """The search behind search_rows / search_batch: query_embeddings fp32 [nq, d] (numpy or tensor) -> (scores fp32
        [nq, k], sidecar rows int64 [nq, k], exactness tally) as numpy + dict, k = top_k clipped to the row count; k = 0 and no
        tally when there is nothing to search (no rows, no queries, a filter nothing passes).  Space 'ip' / 'l2': the first array
        holds the DISTANCES (crs::space_distances), ascending, +inf in empty slots."""
        if self.collection is None:
            raise ValueError("No collection available. Create index first.")
        col = self.collection
        nq = len(query_embeddings)
        nothing = np.zeros((nq, 0), dtype=np.float32), np.zeros((nq, 0), dtype=np.int64), None
        if col.count() == 0 or nq == 0:
            return nothing
        q32 = self._as_f32(query_embeddings).to(col.device).contiguous()
        if q32.shape[1] != col.dim:
            raise ValueError(f"Query dimension {q32.shape[1]} doesn't match the index dimension {col.dim}")
        filt = self._filter_entry(where, where_document)
        if filt is not None and len(filt["rows"]) == 0:
            return nothing
        if col.space != nat.SPACE_COSINE and min(top_k, col.count()) > nat.MAX_K_CERT:
            raise ValueError(f"top_k {top_k} > {nat.MAX_K_CERT} is not supported in space {self.space!r}")
        scores, rows, tally = self._topk_device(q32, min(top_k, col.count()), filt)
        return scores.cpu().numpy(), rows.cpu().numpy(), tally

    def search_rows(self, query_embeddings, top_k: int):
        """search_batch without the sidecar lookup: (scores fp32 [nq, k], sidecar rows int64 [nq, k]) as numpy, best first,
        -1 rows = fewer than k hits.  (retrieve_batch builds its dicts straight from these.)  Space 'ip' / 'l2': distances in
        place of scores, see distances_of."""
        scores, rows, tally = self._search_rows(query_embeddings, top_k)
        if tally is not None:
            self.last_exactness = tally
        return scores, rows

    def distances_of(self, scores) -> np.ndarray:
        """The fp64 distances search / search_batch report for the first array of search_rows: 1 - score in fp32 (cosine); the
        array itself in the spaces whose searches return distances ('ip': 1 - <q, x>, 'l2': sum (q - x)^2, ChromaDB's)."""
        scores = np.asarray(scores, dtype=np.float32)
        if self.space != 'cosine':
            return scores.astype(np.float64)
        return (np.float32(1.0) - scores).astype(np.float64)

    def search_batch(self, query_embeddings, top_k: int = 5, where: Optional[dict] = None,
                     where_document: Optional[dict] = None) -> Dict[str, Any]:
        """Many queries per launch: query_embeddings fp32 [nq, d] (numpy or cuda tensor).
        Same dict as ``search`` with one inner list per query."""
        sh, rh, tally = self._search_rows(query_embeddings, top_k, where, where_document)
        nq = len(query_embeddings)
        if tally is None:
            return {k: [[] for _ in range(max(nq, 1))] for k in _EMPTY}
        self.last_exactness = tally
        col = self.collection
        dist = self.distances_of(sh)                              # one vectorised pass; float(np.float32) per hit was the cost
        ids_l, docs_l, metas_l = col.ids, col.documents, col.metadatas
        out = {'ids': [], 'documents': [], 'metadatas': [], 'distances': []}
        for a in range(nq):
            valid = [r for r in rh[a].tolist() if r >= 0]
            out['ids'].append([ids_l[r] for r in valid])
            out['documents'].append([docs_l[r] for r in valid])
            out['metadatas'].append([metas_l[r] for r in valid])
            out['distances'].append(dist[a, : len(valid)].tolist())
        return out

    # -- management ----------------------------------------------------------------------------
    def delete_collection(self):
        """Delete the collection (frees the slab; removes persisted files)."""
        if self.collection:
            self.collection = None
            self._wire = {}
            self._filters = {}
            self._persisted_rows = None
            if self.persist_directory:
                for path in self._persist_paths().values():
                    if os.path.exists(path):
                        os.remove(path)
                if os.path.isdir(self.persist_directory):
                    self._remove_other_generations(-1)       # every generation's files, a crashed rewrite's included
            self._gen, self._gen_pending, self._docs_bytes = None, False, 0
            logger.info(f"Deleted collection: {self.collection_name}")

    def reset_collection(self):
        """Reset the collection (delete and re-initialise)."""
        self.delete_collection()
        self._initialize_collection()

    def get_stats(self) -> Dict[str, Any]:
        """Collection statistics."""
        if self.collection is None:
            return {"status": "empty", "count": 0}
        try:
            col = self.collection
            elem = 1 if col.slab_type == nat.SLAB_I8 else 2
            return {"name": self.collection_name, "count": col.count(), "metadata": col.metadata,
                    "index_dtype": col.index_dtype, "dimension": col.dim, "rows_on_this_gpu": col.shards[0].n,
                    "rows_per_device": [s.n for s in col.shards],
                    "slab_bytes": int(sum(s.n for s in col.shards) * (col.pdim or 0) * elem)}
        except Exception as e:
            logger.error(f"Failed to get stats: {e}")
            return {"status": "error", "error": str(e)}
