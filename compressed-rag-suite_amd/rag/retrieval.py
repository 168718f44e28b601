"""Context retrieval: embed the query, search the slab, score, threshold, rerank, diversify.

Same class / method names, arguments, return dicts and numeric behaviour as
/root/reference/rag/retrieval.py (``ContextRetriever`` :13-277) -- pinned bit for bit by
tests/golden/retrieve_cases.json, which holds the reference class's own outputs.  The scoring,
lexical rerank and MMR steps are a few hundred scalar operations per query and by default stay on
the host in fp64 Python exactly like the reference; the heavy steps they call (``embed``,
``search``) run on the GPU.  Opt-in, ``mmr_vectors: 'device'``: ``retrieve_batch`` orders the MMR
lists of all its queries with one kernel launch over the store's fp32 rows (csrc/mmr.hip) instead
of the Python loop -- same rule, cosines in fp32 on the device.  Opt-in, ``lexical_rerank: 'device'``:
``retrieve_batch`` scores, thresholds and lexically re-ranks the lists of each device batch with one
kernel launch (csrc/rerank.hip, VectorStore.rerank_lexical) and builds only the surviving dicts --
the host rule in fp64, bit for bit.  Opt-in, ``rerank_model`` (a rag/reranking.py config dict, or a model name): with ``rerank``
on, a BERT cross-encoder scores every (query, chunk text) pair that passed the threshold -- ``rerank_score`` is its score, the list
is sorted on it (stable, descending) and cut to ``top_k``; the search, the ``2 * top_k`` fetch, the threshold and the MMR step
(on ``score``) are as without it.

Opt-in, ``late_interaction`` (a rag/late_interaction.py config dict, or a model name; exclusive with ``rerank_model``): with
``rerank`` on, the lists of every device batch are scored by late interaction (ColBERT's MaxSim) in ONE kernel launch
(csrc/maxsim.hip) over the store's per-token index (VectorStore.token_index: every chunk encoded once, at index time) -- only the
queries are encoded at query time.  ``rerank_score`` is the MaxSim score, the list is sorted on it (stable, descending) and cut to
``top_k``, as with ``rerank_model``; the hybrid lists and ``retrieve``'s filtered lists go through the same scoring.

Opt-in, ``hybrid`` (``true``, or a dict of ``rrf_k``, ``weights``, ``k1``, ``b``): ``retrieve_batch`` fuses the thresholded dense list of every
query with an exact BM25 list over the whole collection (VectorStore.bm25_rows, csrc/bm25.hip) by weighted reciprocal rank fusion
(VectorStore.fuse_rrf, csrc/fuse.hip), so a chunk the encoder ranks far down still surfaces when it matches the query's words;
the re-rank, the cut and the MMR step then run on the fused lists as before.  ``retrieve`` goes through ``retrieve_batch``.
With ``sparse_model`` (a rag/sparse.py config dict, or a model name; needs ``hybrid``) the lexical list is the learned-sparse one
(VectorStore.sparse_rows, csrc/sparse_scan.hip over the SPLADE vectors of every chunk) instead of BM25's.

Additive: ``retrieve_batch`` embeds and searches many queries in one launch each and then applies
the identical per-query post-processing; ``reuse_index_embeddings`` is NOT offered because the
reference re-embeds chunk texts for MMR (:238-239) and near-ties could reorder otherwise.
"""
from __future__ import annotations

import logging
from typing import Dict, List, Optional

import numpy as np

from rag import _search
from rag.indexing import VectorStore
from rag.embedding import EmbeddingModel

logger = logging.getLogger(__name__)


def _kind(model, kind: str) -> dict:
    """The `kind=` keyword ('query' for questions, 'document' for chunk texts) for embedding models that know task prefixes
    (rag.embedding.EmbeddingModel: query_prefix / document_prefix); nothing for a duck-typed model that does not."""
    return {'kind': kind} if hasattr(model, 'query_prefix') else {}


class ContextRetriever:
    """Retrieve relevant context for queries (with re-ranking and diversity mechanisms)."""

    def __init__(self, vector_store: VectorStore, embedding_model: EmbeddingModel, config: dict):
        self.vector_store = vector_store
        self.embedding_model = embedding_model
        self.top_k = config.get('top_k', 3)
        self.similarity_threshold = config.get('similarity_threshold', 0.0)
        self.rerank = config.get('rerank', False)
        self.diversity_penalty = config.get('diversity_penalty', 0.0)
        self.batch_queries = int(config.get('batch_queries', 64))    # additive: queries per launch of retrieve_batch's engine
        # additive: where the MMR step takes the chunks' vectors from.  'reembed' = encode the chunk texts again, as the
        # reference does (rag/retrieval.py:238-239); 'index' = the fp32 rows the store kept when those very texts were
        # indexed (the same encoder's output for the same text: equal up to the rounding of a different batch composition;
        # no tokenisation, no encoder pass); 'auto' = retrieve() re-embeds (reference parity), retrieve_batch() reads the index;
        # 'device' = the index rows again, ordered by ONE kernel launch per retrieve_batch call (VectorStore.mmr_order) instead of
        # the Python loop; lists longer than 64 and stores that cannot serve it (several shards, no fp32 rows) run as 'auto'
        self.mmr_vectors = config.get('mmr_vectors', 'auto')
        if self.mmr_vectors not in ('auto', 'reembed', 'index', 'device'):
            raise ValueError(f"mmr_vectors must be 'auto', 'reembed', 'index' or 'device', got {self.mmr_vectors!r}")
        self.last_mmr = {'mode': 'host', 'lists': 0}      # which path ordered the lists of the last retrieve_batch call
        # additive: where retrieve_batch runs the steps between the search and the MMR step (score, similarity_threshold, the
        # token-overlap re-rank, its stable sort).  'host' = the Python loop below, as the reference; 'device' = ONE kernel launch per
        # device batch (VectorStore.rerank_lexical) with bit-identical results, taken when rerank is on, the metric is cosine and
        # 2 * top_k <= 64; anything else, and a store that answers None, runs as 'host'.  retrieve() always runs on the host
        self.lexical_rerank = config.get('lexical_rerank', 'host')
        if self.lexical_rerank not in ('host', 'device'):
            raise ValueError(f"lexical_rerank must be 'host' or 'device', got {self.lexical_rerank!r}")
        self.last_rerank = {'mode': 'host', 'lists': 0}   # which path scored and re-ranked the lists of the last retrieve_batch call
        # additive: a cross-encoder in place of the token-overlap rule (rag/reranking.py; a config dict, or a string used as its
        # model_name).  Resolved here, so an unknown model fails at construction; used only while `rerank` is on.  Every non-empty
        # list that passed the threshold is scored (also one that needs no cut: its order and rerank_score are the model's), all
        # pairs of a retrieve_batch piece in one predict call; lexical_rerank: 'device' is then not taken
        self.cross_encoder = None
        if config.get('rerank_model'):
            from rag.reranking import CrossEncoderReranker
            self.cross_encoder = CrossEncoderReranker(config['rerank_model'])
        # additive: late interaction in place of the token-overlap rule (rag/late_interaction.py; a config dict, or a string used as
        # its model_name).  Resolved here and attached to the store, whose token index is built on the first re-ranked query (or by
        # VectorStore.token_index()); used only while `rerank` is on; lexical_rerank: 'device' is then not taken
        self.late_interaction = None
        if config.get('late_interaction'):
            if config.get('rerank_model'):
                raise ValueError("late_interaction and rerank_model are exclusive: one model re-ranks a list")
            if not hasattr(vector_store, 'token_index'):
                raise ValueError("late_interaction needs a store with a token index (VectorStore.token_index)")
            from rag.late_interaction import LateInteractionReranker
            self.late_interaction = LateInteractionReranker(config['late_interaction'])
            vector_store.attach_token_encoder(self.late_interaction)
        # additive: hybrid retrieval.  False (default) | True | {'rrf_k': 60, 'weights': [1, 1], 'k1': 1.5, 'b': 0.75}: retrieve_batch
        # fuses each thresholded dense list with the BM25 list of the same query over the whole collection (same `fetch`) by
        # weighted reciprocal rank fusion: fused = w_dense / (rrf_k + i + 1) + w_lex / (rrf_k + j + 1) over the 0-based ranks; 'score'
        # becomes fused / ((w_dense + w_lex) / (rrf_k + 1)), in (0, 1].  lexical_rerank: 'device' is then not taken (its inputs are
        # cosine scores); retrieve() goes through retrieve_batch and refuses metadata filters
        self.hybrid = self._parse_hybrid(config.get('hybrid', False))
        self.last_hybrid = {'lists': 0, 'lexical_only_hits': 0}     # what the last retrieve_batch call fused
        # additive: a learned sparse encoder (rag/sparse.py; a config dict, or a string used as its model_name) in place of BM25 as the
        # lexical list of `hybrid`: VectorStore.sparse_rows instead of bm25_rows (k1 and b are then unused), everything downstream --
        # fusion, the dict keys ('bm25_score' then holds the sparse dot product), thresholds, re-rankers -- unchanged
        self.sparse_encoder = None
        self.last_sparse = {'queries': 0, 'query_terms': 0, 'launches': 0}   # the sparse_rows calls of the last retrieve_batch call
        if config.get('sparse_model'):
            if self.hybrid is None:
                raise ValueError("sparse_model needs hybrid: it replaces the lexical list that hybrid fuses with the dense one")
            if not hasattr(vector_store, 'sparse_rows'):
                raise ValueError("sparse_model needs a store with a sparse index (VectorStore.sparse_rows)")
            from rag.sparse import SparseEncoder
            self.sparse_encoder = SparseEncoder(config['sparse_model'])
            vector_store.attach_sparse_encoder(self.sparse_encoder)
        self._token_sets: Dict[str, frozenset] = {}       # _rerank: text -> its lower-cased token set
        self._engine, self._engine_key = None, None
        self.distance_metric = self._get_distance_metric()
        logger.info(f"Using distance metric: {self.distance_metric}")
        if getattr(embedding_model, 'has_normalize_module', None) is False and getattr(vector_store, 'space', 'cosine') == 'cosine':
            logger.warning("the embedding model's sentence-transformers pipeline has no Normalize module (it is trained for dot-product "
                           "scoring, where the length of a vector carries relevance) but the vector store ranks by cosine: consider "
                           "vector_store space 'ip' with embedding normalize False")

    @staticmethod
    def _parse_hybrid(value) -> Optional[dict]:
        """The `hybrid` config value as {'rrf_k', 'weights', 'k1', 'b'} floats, or None when off; anything else raises ValueError."""
        if value is None or value is False:
            return None
        out = {'rrf_k': 60.0, 'weights': (1.0, 1.0), 'k1': 1.5, 'b': 0.75}
        if value is True:
            return out
        if not isinstance(value, dict):
            raise ValueError(f"hybrid must be false, true or a dict of rrf_k / weights / k1 / b, got {value!r}")
        unknown = sorted(set(value) - set(out))
        if unknown:
            raise ValueError(f"hybrid: unknown key(s) {unknown}; known: b, k1, rrf_k, weights")

        def number(key, lo, hi):
            v = value[key]
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not (lo <= float(v) <= hi):
                raise ValueError(f"hybrid: {key} must be a number in [{lo}, {hi}], got {v!r}")
            return float(v)
        if 'rrf_k' in value:
            out['rrf_k'] = number('rrf_k', 0.0, 1e9)
        if 'k1' in value:
            out['k1'] = number('k1', 0.0, 1e6)
        if 'b' in value:
            out['b'] = number('b', 0.0, 1.0)
        if 'weights' in value:
            w = value['weights']
            if (not isinstance(w, (list, tuple)) or len(w) != 2
                    or any(isinstance(x, bool) or not isinstance(x, (int, float)) or not (0.0 <= float(x) <= 1e9) for x in w)
                    or float(w[0]) + float(w[1]) <= 0.0):
                raise ValueError(f"hybrid: weights must be two numbers >= 0 (dense, lexical), not both 0, got {w!r}")
            out['weights'] = (float(w[0]), float(w[1]))
        return out

    def _get_distance_metric(self) -> str:
        """The store's space: the collection's hnsw:space, or what the store is configured to create it with."""
        try:
            collection = self.vector_store.collection
            if collection:
                return collection.metadata.get('hnsw:space', 'cosine')
        except Exception:
            pass
        return getattr(self.vector_store, 'space', 'cosine')     # no collection yet: the space the store will create it with

    # ---- scoring ---------------------------------------------------------------------------------
    def _distance_to_similarity(self, distance: float) -> float:
        """Map a store distance to a [0, 1] score.  The cosine branch is the reference's
        ``1 - d^2/2`` with d clamped to [0, 2] (its :75-77), applied to d = 1 - cos as returned by
        the store: that IS the reference's ``score``, so it is kept as is."""
        metric = self.distance_metric
        if metric == 'cosine':
            d = max(0.0, min(2.0, distance))
            return max(0.0, min(1.0, 1.0 - (d * d / 2.0)))
        if metric == 'l2':
            return 1.0 / (1.0 + distance)
        if metric == 'ip':
            return max(0.0, min(1.0, (distance + 2.0) / 2.0))
        logger.warning(f"Unknown distance metric: {metric}, using default conversion")
        return max(0.0, 1.0 - (distance / 2.0))

    def _store_distances(self, sc) -> np.ndarray:
        """The fp64 distances of the first array of VectorStore.search_rows: 1 - score in fp32 for cosine; a store of space
        'ip' / 'l2' returns its distances there and converts them itself (VectorStore.distances_of)."""
        store = self.vector_store
        if hasattr(store, 'distances_of'):
            return store.distances_of(sc)
        return (np.float32(1.0) - sc.astype(np.float32)).astype(np.float64)

    def _hits_to_chunks(self, ids, documents, metadatas, distances) -> List[Dict]:
        chunks = []
        for pos, chunk_id in enumerate(ids):
            distance = distances[pos]
            item = {
                'text': documents[pos],
                'score': self._distance_to_similarity(distance),
                'distance': distance,
                'metadata': metadatas[pos] if metadatas else {},
                'chunk_id': chunk_id,
            }
            if item['score'] >= self.similarity_threshold:
                chunks.append(item)
        return chunks

    def _post_process(self, query: str, chunks: List[Dict], k: int) -> List[Dict]:
        if not chunks:
            logger.warning(f"No chunks passed similarity threshold of {self.similarity_threshold}")
            return []
        if self.rerank and self.cross_encoder is not None:
            chunks = self._rerank_cross([query], [chunks], k)[0]
            self.last_rerank = {'mode': 'cross-encoder', 'lists': 1}
        elif self.rerank and self.late_interaction is not None:
            chunks = self._rerank_late([query], [chunks], k, self._rows_of_chunks(chunks))[0]
            self.last_rerank = {'mode': 'late-interaction', 'lists': 1}
        elif self.rerank and len(chunks) > k:
            chunks = self._rerank(query, chunks, k)
        else:
            chunks = chunks[:k]
        if self.diversity_penalty > 0 and len(chunks) > 1:
            chunks = self._apply_diversity(chunks)
        return chunks

    # ---- public ----------------------------------------------------------------------------------
    def retrieve(self, query: str, top_k: Optional[int] = None, filters: Optional[dict] = None) -> List[Dict]:
        """List of dicts with 'text', 'score', 'distance', 'metadata', 'chunk_id' (+ 'rerank_score'
        when re-ranked), at most k of them."""
        k = top_k or self.top_k
        if self.hybrid is not None:
            if filters is not None:
                raise ValueError("hybrid retrieval does not take metadata filters: the lexical list is not filtered")
            return self.retrieve_batch([query], top_k=top_k)[0]
        if self.late_interaction is not None and self.rerank and filters is None:
            return self.retrieve_batch([query], top_k=top_k)[0]
        try:
            query_embedding = self.embedding_model.embed(query, **_kind(self.embedding_model, 'query'))
            results = self.vector_store.search(query_embedding=query_embedding,
                                               top_k=k * 2 if self.rerank else k, where=filters)
            if not results['ids'][0]:
                logger.warning("No results found for query")
                return []
            metas = results['metadatas'][0] if results['metadatas'] else None
            chunks = self._hits_to_chunks(results['ids'][0], results['documents'][0], metas,
                                          results['distances'][0])
            if self.mmr_vectors in ('index', 'device') and self.diversity_penalty > 0:
                return self.retrieve_batch([query], top_k=top_k)[0] if filters is None else self._post_process(query, chunks, k)
            return self._post_process(query, chunks, k)
        except Exception as e:
            logger.error(f"Retrieval failed: {e}")
            raise

    # ---- batched retrieval (additive; the reference has no batched entry point) --------------------------------------
    def _engine_for(self, fetch: int, seq: int, n_batches: int = 0):
        """The throughput engine (rag/_engine.py: role lanes, hipGraph replay, several batches in flight) for this store /
        encoder pair, or None when the store's layout needs the general path (several shards, filters, top_k > 64)."""
        store, model = self.vector_store, self.embedding_model
        view = store.engine_view() if hasattr(store, "engine_view") else None
        enc = getattr(model, "model", None)
        if view is None or enc is None or fetch > 64 or not getattr(model, "normalize", True):
            return None
        # one encoder forward serves a group of batches (rag/_engine.py): never more of them than a call of this size brings
        cap = 1 << (max(1, n_batches).bit_length() - 1)
        # mutation_epoch: an in-place update leaves n and the slab pointer as they were, but the engine's graphs hold the OLD row_err_max
        key = (fetch, seq, view.n, int(view.slab.data_ptr()), self.batch_queries, min(cap, 16), getattr(store, "mutation_epoch", 0))
        if self._engine_key != key:
            from rag._engine import RetrievalEngine
            self._engine = RetrievalEngine(enc, view, self.batch_queries, seq, fetch, k_scan=store.refine_overfetch,
                                           refine=view.shadow is not None, exact=store.refine_exact, exact_cap=store.exact_cap,
                                           group_cap=cap)
            self._engine_key = key
        return self._engine

    def _search_many(self, queries: List[str], fetch: int):
        """Generator over PIECES of the query list, in order: each piece a list of per-query (scores fp32 [<= fetch], sidecar rows
        int64 [<= fetch]) numpy arrays, best first (or, once, a duck-typed store's search_batch dict).  With the throughput
        engine a piece is one device batch, yielded as soon as it is through -- the caller builds that batch's dicts while the
        device works on the following ones."""
        import numpy as _np
        model, store = self.embedding_model, self.vector_store
        qb = self.batch_queries
        eng = None
        if len(queries) >= qb and hasattr(store, 'engine_view') and store.collection is not None and store.collection.count() > 0:
            token_ids = model.tokenize(list(queries), **_kind(model, 'query'))
            longest = max(len(t) for t in token_ids)
            seq = next((st for st in (16, 32, 64) if longest <= st and st <= model.shape.max_seq), None)
            eng = self._engine_for(min(fetch, store.collection.count()), seq, -(-len(queries) // qb)) if seq else None
        if eng is None:                       # general path: one encoder pass + one search launch for the whole list
            emb = (model.embed_device(list(queries), **_kind(model, 'query')) if hasattr(model, "embed_device")
                   else model.embed(list(queries), **_kind(model, 'query')))
            if not hasattr(store, "search_rows"):          # any store with the additive search_batch (duck-typed)
                yield store.search_batch(emb, top_k=fetch)
                return
            scores, rows = store.search_rows(emb, fetch)
            yield [(scores[i], rows[i]) for i in range(len(queries))]
            return
        pad = getattr(model.tokenizer, "pad_id", 0)

        def batches():
            for lo in range(0, len(token_ids), qb):
                ids = _np.full((min(qb, len(token_ids) - lo), eng.seq), pad, dtype=_np.int32)
                lens = _np.empty(ids.shape[0], dtype=_np.int32)
                for r, t in enumerate(token_ids[lo:lo + qb]):
                    ids[r, :len(t)] = t
                    lens[r] = len(t)
                yield ids, lens

        total = None
        for s, r, st, q_over in eng.search_token_batches(batches(), overflow_queries=True):
            tally = _search.tally(st, len(st), eng.k, eng.refine, eng.exact)
            if q_over is not None:
                # status 2 (more rows in a query's band than the engine's escalation list holds): the store's own search
                # repeats those queries with longer lists, as search_batch does; they count by their final status
                over = np.nonzero(st == 2)[0]
                s, r = s.copy(), r.copy()
                s[over], r[over], again = store._search_rows(q_over, s.shape[1])
                tally = _search.retried_tally(tally, again)
            total = tally if total is None else _search.add_tallies(total, tally)
            yield [(s[i], r[i]) for i in range(s.shape[0])]
        store.last_exactness = total

    def retrieve_batch(self, queries: List[str], top_k: Optional[int] = None) -> List[List[Dict]]:
        """``[retrieve(q) for q in queries]`` for many queries at once: the encoder forwards and scans of the whole list
        run through the throughput engine (Qb = ``batch_queries`` per launch, several launches in flight), scoring and the
        threshold are vectorised (same fp64 arithmetic as ``_distance_to_similarity``), and the MMR step re-embeds the chunk
        texts of ALL queries in one encoder pass (the reference re-embeds per query, rag/retrieval.py:238-239).
        Same dicts, same order as ``retrieve`` up to the rounding of batched encoder forwards."""
        k = top_k or self.top_k
        if not queries:
            return []
        store = self.vector_store
        col = store.collection
        if col is None:
            raise ValueError("No collection available. Create index first.")
        fetch = k * 2 if self.rerank else k
        hybrid = self.hybrid
        if hybrid is not None:
            if fetch > 64:
                raise ValueError(f"hybrid retrieval fetches at most 64 rows per list, got {fetch} (top_k {k}, rerank {bool(self.rerank)})")
            if not (hasattr(store, 'bm25_rows') and hasattr(store, 'fuse_rrf') and hasattr(store, 'search_rows')):
                raise ValueError("hybrid retrieval needs a store with search_rows, bm25_rows and fuse_rrf")
            self.last_hybrid = {'lists': 0, 'lexical_only_hits': 0}
            self.last_sparse = {'queries': 0, 'query_terms': 0, 'launches': 0}
        per_query: List[List[Dict]] = []
        row_of: Dict[int, int] = {}           # id(chunk dict) -> sidecar row (our store only)
        ids_l, docs_l, metas_l = getattr(col, 'ids', None), getattr(col, 'documents', None), getattr(col, 'metadatas', None)
        queries = list(queries)
        cross = self.cross_encoder if self.rerank else None
        late = self.late_interaction if self.rerank else None
        if late is not None and ids_l is None:
            raise ValueError("late_interaction needs a store that returns sidecar rows (search_rows)")
        on_device = (self.lexical_rerank == 'device' and bool(self.rerank) and self.distance_metric == 'cosine' and fetch <= 64
                     and ids_l is not None and hasattr(store, 'rerank_lexical') and cross is None and late is None and hybrid is None)
        host_pieces = 0
        for piece in self._search_many(queries, fetch):      # one device batch at a time: its dicts are built while the next ones run
            piece_start = len(per_query)
            if hybrid is not None:
                if isinstance(piece, dict):
                    raise ValueError("hybrid retrieval needs a store with search_rows, bm25_rows and fuse_rrf")
                host_pieces += 1
                piece_queries = queries[piece_start:piece_start + len(piece)]
                for query, chunks in zip(piece_queries, self._hybrid_lists(piece_queries, piece, fetch, row_of)):
                    if chunks and cross is None and late is None:
                        chunks = self._rerank(query, chunks, k) if self.rerank and len(chunks) > k else chunks[:k]
                    per_query.append(chunks)
                if cross is not None:
                    per_query[piece_start:] = self._rerank_cross(piece_queries, per_query[piece_start:], k)
                elif late is not None:
                    per_query[piece_start:] = self._rerank_late(piece_queries, per_query[piece_start:], k, row_of)
                continue
            if on_device and not isinstance(piece, dict):
                built = self._rerank_on_device(queries[len(per_query):len(per_query) + len(piece)], piece, k, row_of)
                if built is not None:
                    per_query.extend(built)
                    continue
            host_pieces += 1
            if isinstance(piece, dict):       # a duck-typed store's search_batch dict: lists per query
                ids_l = docs_l = metas_l = None
                piece = [(np.asarray(piece['distances'][p], dtype=np.float64), (piece['ids'][p], piece['documents'][p],
                          piece['metadatas'][p] if piece.get('metadatas') else None)) for p in range(len(queries))]
            for sc, rows in piece:
                query = queries[len(per_query)]
                if ids_l is None:
                    dist, (h_ids, h_docs, h_metas) = sc, rows
                    rows = np.arange(len(h_ids))
                else:
                    valid = rows >= 0
                    rows, sc = rows[valid], sc[valid]
                    dist = self._store_distances(sc)                                     # the store's distances, as search() returns them
                    h_ids, h_docs, h_metas = ids_l, docs_l, metas_l
                if rows.size == 0:
                    logger.warning("No results found for query")
                    per_query.append([])
                    continue
                if self.distance_metric == 'cosine':                                          # _distance_to_similarity, vectorised (same fp64 ops)
                    d = np.minimum(np.maximum(dist, 0.0), 2.0)
                    score = np.minimum(np.maximum(1.0 - (d * d / 2.0), 0.0), 1.0)
                else:
                    score = np.array([self._distance_to_similarity(float(x)) for x in dist])
                keep = score >= self.similarity_threshold
                chunks = [{'text': h_docs[r], 'score': float(s_), 'distance': float(d_), 'metadata': h_metas[r] if h_metas else {},
                           'chunk_id': h_ids[r]}
                          for r, s_, d_, ok in zip(rows.tolist(), score.tolist(), dist.tolist(), keep.tolist()) if ok]
                if ids_l is not None:
                    for c_, r_ in zip(chunks, [r for r, ok in zip(rows.tolist(), keep.tolist()) if ok]):
                        row_of[id(c_)] = r_
                if not chunks:
                    logger.warning(f"No chunks passed similarity threshold of {self.similarity_threshold}")
                    per_query.append([])
                    continue
                if cross is None and late is None:        # (a model takes the whole piece at once, below)
                    chunks = self._rerank(query, chunks, k) if self.rerank and len(chunks) > k else chunks[:k]
                per_query.append(chunks)
            if cross is not None:
                per_query[piece_start:] = self._rerank_cross(queries[piece_start:len(per_query)], per_query[piece_start:], k)
            elif late is not None:                    # (ids_l is not None: checked before the loop)
                per_query[piece_start:] = self._rerank_late(queries[piece_start:len(per_query)], per_query[piece_start:], k, row_of)
        self.last_rerank = {'mode': 'cross-encoder' if cross is not None else 'late-interaction' if late is not None
                            else 'device' if on_device and not host_pieces else 'host',
                            'lists': len(per_query) if self.rerank else 0}
        self.last_mmr = {'mode': 'host', 'lists': sum(1 for chunks in per_query if len(chunks) > 1) if self.diversity_penalty > 0 else 0}
        # the MMR kernel reads the store's fp32 rows as they are stored: cosine only (as the lexical kernel above); in the other
        # spaces 'device' falls back to 'index', whose rows_f32 returns the caller's vectors
        if (self.diversity_penalty > 0 and self.mmr_vectors == 'device' and self.distance_metric == 'cosine' and ids_l is not None
                and self._mmr_on_device(per_query, row_of)):
            return per_query
        from_index = self.mmr_vectors in ('auto', 'index', 'device') and ids_l is not None and hasattr(store, 'rows_f32')
        if self.diversity_penalty > 0 and from_index:
            # the chunks' vectors straight from the index (one gather for the whole batch), then the reference's greedy MMR
            need = sorted({row_of[id(c)] for chunks in per_query if len(chunks) > 1 for c in chunks})
            vecs = store.rows_f32(need) if need else None
            if vecs is None:
                from_index = False
            else:
                at = {r: p for p, r in enumerate(need)}
                per_query = [self._apply_diversity(chunks, vectors=vecs[[at[row_of[id(c)]] for c in chunks]])
                             if len(chunks) > 1 else chunks for chunks in per_query]
        if self.diversity_penalty > 0 and not from_index:
            # ONE encoder pass for the chunk texts of every query (deduplicated), then the reference's greedy MMR per query
            texts, index = [], {}
            for chunks in per_query:
                if len(chunks) > 1:
                    for c in chunks:
                        if c['text'] not in index:
                            index[c['text']] = len(texts)
                            texts.append(c['text'])
            if texts:
                vectors = self.embedding_model.embed(texts, **_kind(self.embedding_model, 'document'))
                per_query = [self._apply_diversity(chunks, vectors=vectors[[index[c['text']] for c in chunks]])
                             if len(chunks) > 1 else chunks for chunks in per_query]
        return per_query

    def _hybrid_lists(self, queries: List[str], piece, fetch: int, row_of: Dict[int, int]) -> List[List[Dict]]:
        """The fused chunk lists of one piece of _search_many (per query: scores fp32, sidecar rows int64, best first): the dense
        lists go through the cosine score and similarity_threshold as in retrieve_batch's host loop, VectorStore.bm25_rows gives
        the lexical lists of the same queries (same `fetch`), and ONE VectorStore.fuse_rrf call fuses each pair to at most
        `fetch` rows.  A dict carries 'score' = fused / ((w_dense + w_lex) / (rrf_k + 1)), 'distance' (None for a lexical-only hit),
        'dense_score' (the cosine-mapped score or None), 'bm25_score' (0.0 when absent), 'dense_rank' / 'lexical_rank' (or None)."""
        store, hy = self.vector_store, self.hybrid
        col = store.collection
        nq = len(piece)
        m_dense = max(1, max((len(sc) for sc, _ in piece), default=1))
        dense = np.full((nq, m_dense), -1, dtype=np.int64)
        d_dist = np.zeros((nq, m_dense), dtype=np.float64)
        d_score = np.zeros((nq, m_dense), dtype=np.float64)
        for i, (sc, rows) in enumerate(piece):
            valid = rows >= 0
            rows, sc = rows[valid], sc[valid]
            dist = self._store_distances(sc)                                       # the store's distances, as search() returns them
            if self.distance_metric == 'cosine':                                      # _distance_to_similarity, vectorised (same fp64 ops)
                d = np.minimum(np.maximum(dist, 0.0), 2.0)
                score = np.minimum(np.maximum(1.0 - (d * d / 2.0), 0.0), 1.0)
            else:
                score = np.array([self._distance_to_similarity(float(x)) for x in dist], dtype=np.float64)
            keep = score >= self.similarity_threshold
            n = int(keep.sum())
            dense[i, :n], d_dist[i, :n], d_score[i, :n] = rows[keep], dist[keep], score[keep]
        if self.sparse_encoder is not None:
            lex_scores, lex_rows = store.sparse_rows(queries, fetch)
            ran = store.last_sparse
            self.last_sparse = {'queries': self.last_sparse['queries'] + ran['queries'], 'query_terms': ran['query_terms'],
                                'launches': self.last_sparse['launches'] + ran['launches']}
        else:
            lex_scores, lex_rows = store.bm25_rows(queries, fetch, k1=hy['k1'], b=hy['b'])
        w_dense, w_lex = hy['weights']
        rows, fused, dpos, lpos, count = store.fuse_rrf(dense, lex_rows, fetch, c=hy['rrf_k'], weights=(w_dense, w_lex))
        norm = (w_dense + w_lex) / (hy['rrf_k'] + 1.0)
        ids_l, docs_l, metas_l = col.ids, col.documents, col.metadatas
        out = []
        for i in range(nq):
            n = int(count[i])
            chunks = []
            for r, f, dp, lp in zip(rows[i, :n].tolist(), fused[i, :n].tolist(), dpos[i, :n].tolist(), lpos[i, :n].tolist()):
                c_ = {'text': docs_l[r], 'score': f / norm, 'distance': float(d_dist[i, dp]) if dp >= 0 else None,
                      'metadata': metas_l[r] if metas_l else {}, 'chunk_id': ids_l[r],
                      'dense_score': float(d_score[i, dp]) if dp >= 0 else None,
                      'bm25_score': float(lex_scores[i, lp]) if lp >= 0 else 0.0,
                      'dense_rank': dp if dp >= 0 else None, 'lexical_rank': lp if lp >= 0 else None}
                row_of[id(c_)] = r
                chunks.append(c_)
                if dp < 0:
                    self.last_hybrid['lexical_only_hits'] += 1
            if not chunks:
                logger.warning("No results found for query")
            self.last_hybrid['lists'] += 1
            out.append(chunks)
        return out

    def _rerank_on_device(self, queries: List[str], piece, k: int, row_of: Dict[int, int]) -> Optional[List[List[Dict]]]:
        """The chunk lists of one piece of _search_many (per query: scores fp32, sidecar rows int64, best first), scored,
        thresholded and lexically re-ranked by ONE VectorStore.rerank_lexical call: a padded [queries, longest] block up, the
        order, scores and re-rank scores back, and only the surviving <= k dicts per query built -- the keys and values the host
        loop of retrieve_batch produces.  None (nothing done) when a list is longer than 64 or the store answers None."""
        col = self.vector_store.collection
        m_max = max((len(sc) for sc, _ in piece), default=0)
        if not 1 <= m_max <= 64:
            return None
        scores = np.zeros((len(piece), m_max), dtype=np.float32)
        rows = np.full((len(piece), m_max), -1, dtype=np.int64)
        for i, (sc, r) in enumerate(piece):
            scores[i, :len(sc)], rows[i, :len(r)] = sc, r
        got = self.vector_store.rerank_lexical(queries, scores, rows, k, self.similarity_threshold)
        if got is None:
            return None
        order, count, sim, rr, reranked = got
        dist = (np.float32(1.0) - scores).astype(np.float64)         # the store's distances, as search() returns them
        ids_l, docs_l, metas_l = col.ids, col.documents, col.metadatas
        out = []
        for i in range(len(piece)):
            n = int(count[i])
            if n == 0:
                logger.warning("No results found for query" if not (rows[i] >= 0).any()
                               else f"No chunks passed similarity threshold of {self.similarity_threshold}")
                out.append([])
                continue
            at = order[i, :n].tolist()
            r_i, s_i, d_i = rows[i, at].tolist(), sim[i, at].tolist(), dist[i, at].tolist()
            chunks = [{'text': docs_l[r], 'score': s_, 'distance': d_, 'metadata': metas_l[r] if metas_l else {}, 'chunk_id': ids_l[r]}
                      for r, s_, d_ in zip(r_i, s_i, d_i)]
            if reranked[i]:
                for c_, v in zip(chunks, rr[i, at].tolist()):
                    c_['rerank_score'] = v
            for c_, r in zip(chunks, r_i):
                row_of[id(c_)] = r
            out.append(chunks)
        return out

    def _mmr_on_device(self, per_query: List[List[Dict]], row_of: Dict[int, int]) -> bool:
        """Re-order, in place, every list of `per_query` with more than one chunk by the store's MMR kernel: one padded
        [lists, longest] block of sidecar rows and fp64 scores, one VectorStore.mmr_order call.  False (nothing changed) when a
        list is longer than the kernel's 64 or the store answers None: the caller goes on with the host path."""
        store = self.vector_store
        todo = [p for p, chunks in enumerate(per_query) if len(chunks) > 1]
        if not todo:
            return True
        m_max = max(len(per_query[p]) for p in todo)
        if m_max > 64 or not hasattr(store, 'mmr_order'):
            return False
        rows = np.full((len(todo), m_max), -1, dtype=np.int64)
        rel = np.zeros((len(todo), m_max), dtype=np.float64)
        counts = np.empty(len(todo), dtype=np.int32)
        for i, p in enumerate(todo):
            chunks = per_query[p]
            counts[i] = len(chunks)
            rows[i, :len(chunks)] = [row_of[id(c)] for c in chunks]
            rel[i, :len(chunks)] = [c['score'] for c in chunks]
        order = store.mmr_order(rows, rel, counts, 1.0 - self.diversity_penalty)
        if order is None:
            return False
        for i, p in enumerate(todo):
            chunks = per_query[p]
            per_query[p] = [chunks[j] for j in order[i, :len(chunks)].tolist()]
        self.last_mmr = {'mode': 'device', 'lists': len(todo)}
        return True

    def get_context_string(self, query: str, top_k: Optional[int] = None, separator: str = "\n\n") -> str:
        chunks = self.retrieve(query, top_k=top_k)
        return separator.join(chunk['text'] for chunk in chunks) if chunks else ""

    # ---- rerank / diversity ----------------------------------------------------------------------
    TOKEN_SET_CACHE_CAP = 65536       # entries; the cache is dropped whole when it passes this

    def _tokens_of(self, text: str) -> frozenset:
        """set(text.lower().split()), kept per text string: the same chunks come back for query after query.  Keyed by the
        text itself, so a deleted, updated or upserted chunk can never meet another text's set."""
        cache = self._token_sets
        got = cache.get(text)
        if got is None:
            if len(cache) >= self.TOKEN_SET_CACHE_CAP:
                cache.clear()
            got = cache[text] = frozenset(text.lower().split())
        return got

    def _rerank(self, query: str, chunks: List[Dict], top_k: int) -> List[Dict]:
        """70 % semantic score + 30 % fraction of query tokens present in the chunk."""
        wanted = set(query.lower().split())
        norm = max(len(wanted), 1)
        for chunk in chunks:
            hits = len(wanted & self._tokens_of(chunk['text']))
            chunk['rerank_score'] = chunk['score'] * 0.7 + (hits / norm) * 0.3
        chunks.sort(key=lambda c: c.get('rerank_score', c['score']), reverse=True)
        return chunks[:top_k]

    def _rerank_cross(self, queries: List[str], lists: List[List[Dict]], top_k: int) -> List[List[Dict]]:
        """The cross-encoder in place of _rerank, for the chunk lists of several queries at once: ONE predict call over every
        (query, chunk text) pair, rerank_score = the model's score, each list sorted on it (stable, descending) and cut."""
        pairs = [(q, c['text']) for q, chunks in zip(queries, lists) for c in chunks]
        if not pairs:
            return [chunks[:top_k] for chunks in lists]
        scores = self.cross_encoder.predict(pairs).tolist()
        out, at = [], 0
        for chunks in lists:
            for c in chunks:
                c['rerank_score'] = scores[at]
                at += 1
            out.append(sorted(chunks, key=lambda c: c['rerank_score'], reverse=True)[:top_k])
        return out

    def _rows_of_chunks(self, chunks: List[Dict]) -> Dict[int, int]:
        """id(chunk dict) -> sidecar row for chunks that came back from VectorStore.search (retrieve's filtered path): the row
        whose id is the chunk's and whose document is its text (create_index accepts duplicate ids)."""
        col = self.vector_store.collection
        idmap = col._id_rows()
        out = {}
        for c in chunks:
            rows = idmap.get(c['chunk_id'], [])
            out[id(c)] = next((r for r in rows if col.documents[r] == c['text']), rows[0] if rows else -1)
        return out

    def _rerank_late(self, queries: List[str], lists: List[List[Dict]], top_k: int, row_of: Dict[int, int]) -> List[List[Dict]]:
        """Late interaction in place of _rerank, for the chunk lists of several queries at once: ONE LateInteractionReranker.score_rows
        call (the queries' encoder forward + one crs_maxsim launch over the store's token index) for a padded [queries, longest]
        block of sidecar rows; rerank_score = the MaxSim score, each list sorted on it (stable, descending) and cut."""
        m_max = max((len(chunks) for chunks in lists), default=0)
        if m_max == 0:
            return [chunks[:top_k] for chunks in lists]
        rows = np.full((len(lists), m_max), -1, dtype=np.int64)
        for i, chunks in enumerate(lists):
            rows[i, :len(chunks)] = [row_of[id(c)] for c in chunks]
        scores = self.late_interaction.score_rows(queries, rows, self.vector_store).cpu().numpy()
        out = []
        for i, chunks in enumerate(lists):
            for c, v in zip(chunks, scores[i, :len(chunks)].tolist()):
                c['rerank_score'] = v
            out.append(sorted(chunks, key=lambda c: c['rerank_score'], reverse=True)[:top_k])
        return out

    def _apply_diversity(self, chunks: List[Dict], vectors=None) -> List[Dict]:
        """Greedy maximal-marginal-relevance re-ordering over re-embedded chunk texts:
        value = lambda * score - (1 - lambda) * max(0, max cos to the already selected).
        `vectors` (retrieve_batch): the chunks' embeddings, already at hand for the whole batch.

        Same values as the reference's triple loop (rag/retrieval.py:246-275), computed once each: the reference
        re-evaluates cos(candidate, chosen) for every chosen chunk in every round (~k^3/3 dot products and twice as many
        norms); a candidate's running maximum only ever changes by the newest chosen chunk, and max() of floats does not
        depend on the order it is taken in, so one cos per (candidate, newly chosen) pair -- k^2/2 -- gives bit-identical
        `closest`, `value` and order (pinned by tests/golden/retrieve_cases.json)."""
        if len(chunks) <= 1:
            return chunks
        lam = 1.0 - self.diversity_penalty
        if vectors is None:
            vectors = self.embedding_model.embed([c['text'] for c in chunks], **_kind(self.embedding_model, 'document'))
        norms = [np.linalg.norm(v) for v in vectors]
        order = [0]
        pending = list(range(1, len(chunks)))
        closest = {cand: 0.0 for cand in pending}
        newest = 0
        while pending and len(order) < len(chunks):
            winner, winner_value = None, -float('inf')
            for cand in pending:
                cos = np.dot(vectors[cand], vectors[newest]) / (norms[cand] * norms[newest])
                closest[cand] = max(closest[cand], cos)
                value = lam * chunks[cand]['score'] - (1 - lam) * closest[cand]
                if value > winner_value:
                    winner, winner_value = cand, value
            if winner is None:
                break
            order.append(winner)
            pending.remove(winner)
            newest = winner
        return [chunks[i] for i in order]
