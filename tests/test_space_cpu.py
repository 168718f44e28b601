"""CPU: the inner-product / squared-L2 transform (tests/_space_ref.py restates csrc/space.hip in numpy), the store's configuration
rules for the spaces, the new entry points of the library, and the retriever's 'ip' / 'l2' scoring branches."""
import ctypes
import logging
import os
import re

import numpy as np
import pytest

import _space_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("crs_space_row_dim", "crs_rows_norm_max", "crs_slab_append_space_f32", "crs_slab_write_rows_space_f32",
       "crs_slab_rescale_space", "crs_queries_to_space", "crs_space_distances")


def _rows(n=600, d=96, seed=3, spread=7.0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d))
    x *= np.exp(rng.uniform(0.0, np.log(spread), size=(n, 1))) / np.sqrt((x * x).sum(axis=1, keepdims=True))
    return x.astype(np.float32)


@pytest.mark.parametrize("space", sr.SPACES)
def test_recover_is_bit_exact(space):
    x = _rows()
    R = sr.norm_scale_for(sr.row_norm_max(x))
    assert R == 8.0 and sr.norm_scale_for(8.0) == 8.0 and sr.norm_scale_for(8.000001) == 16.0 and sr.norm_scale_for(0.3) == 0.5
    for scale in (R, 4 * R, 1024 * R):
        rows = sr.store_rows(x, space, scale)
        assert rows.dtype == np.float32 and rows.shape == (len(x), x.shape[1] + (space == "l2"))
        assert np.array_equal(sr.recover(rows, space, scale).view(np.uint32), x.view(np.uint32))
        norm2 = (rows.astype(np.float64) ** 2).sum(axis=1)
        assert norm2.max() <= (1.0 if space == "ip" else 0.25 + 1.0 / 16) * (1 + 1e-6)


@pytest.mark.parametrize("space", sr.SPACES)
@pytest.mark.parametrize("shift", [1, 2, 5])
def test_rescaled_rows_equal_freshly_stored_rows(space, shift):
    x = _rows(seed=5)
    R = sr.norm_scale_for(sr.row_norm_max(x))
    grown = sr.rescale_rows(sr.store_rows(x, space, R), space, shift)
    fresh = sr.store_rows(x, space, R * 2.0 ** shift)
    assert np.array_equal(grown.view(np.uint32), fresh.view(np.uint32))


@pytest.mark.parametrize("space", sr.SPACES)
def test_ranking_of_transformed_rows_is_the_metric_ranking(space):
    d, k = 96, 10
    x = sr.make_rows(1500, d, seed=9)
    R = sr.norm_scale_for(sr.row_norm_max(x))
    q = sr.pick_queries(x, space, R, 32, (k,), seed=10, pool=512)
    metric = sr.metric64(q, x, space)
    tol = sr.swap_tol(q, d, space, R)
    assert (sr.kth_gaps(metric, (k,)) > tol[:, None]).all()
    scores = sr.queries(q, space, R) @ sr.store_rows(x, space, R).astype(np.float64).T       # what the scan ranks, in fp64
    got = np.stack([sr.ranking(-scores[r])[:k] for r in range(len(q))])
    if space == "ip":      # an exact scaling of both sides: the very same order
        assert np.array_equal(got, np.stack([sr.ranking(metric[r])[:k] for r in range(len(q))]))
    assert sr.topk_errors(got, metric, k, tol) == {}
    # the identity behind l2: |q - x|^2 = |q|^2 - 4 R^2 (p . v - |v|^2), p = q / R
    if space == "l2":
        v = sr.store_rows(x, space, R).astype(np.float64)
        p = q.astype(np.float64) / R
        ident = (q.astype(np.float64) ** 2).sum(axis=1)[:, None] - 4 * R * R * (p @ v[:, :-1].T - v[:, -1][None, :])
        assert np.abs(ident - metric).max() < 1e-5


def test_config_validation_and_refusals():
    from rag.indexing import SlabCollection, VectorStore
    assert VectorStore({}).space == "cosine"
    for space in ("ip", "l2"):
        assert VectorStore({"space": space}).space == space
        assert SlabCollection("c", "fp16", True, ["cpu"], space).metadata == {"hnsw:space": space}
    assert SlabCollection("c", "fp16", True, ["cpu"]).metadata == {"hnsw:space": "cosine"}
    for bad in ("dot", "L2", None, 1):
        with pytest.raises(ValueError, match="space must be"):
            VectorStore({"space": bad})
    for space in ("ip", "l2"):
        with pytest.raises(ValueError, match="refine_fp32"):
            VectorStore({"space": space, "refine_fp32": False})
        for cfg, layout in (({"sharded": True}, "sharded=True"), ({"num_gpus": 2}, "num_gpus > 1"), ({"devices": ["cuda:0", "cuda:1"]}, "devices")):
            with pytest.raises(NotImplementedError, match=re.escape(layout)):
                VectorStore({"space": space, **cfg})
    VectorStore({"space": "cosine", "refine_fp32": False})          # the cosine store keeps every layout it had
    VectorStore({"space": "cosine", "sharded": True})


def test_engine_refuses_the_spaces():
    from rag import _native as nat
    from rag._engine import RetrievalEngine
    from rag._search import ShardView
    for space in (nat.SPACE_IP, nat.SPACE_L2):
        with pytest.raises(ValueError, match="cosine stores only"):
            RetrievalEngine(None, ShardView(None, None, None, 0, 8, nat.SLAB_F16, space=space), 16, 16, 10)


def test_pipeline_section_reaches_the_store():
    import inspect
    from rag.pipeline import RAGPipeline
    assert "VectorStore(section('vector_store', {}))" in inspect.getsource(RAGPipeline.setup)


def test_symbols_are_declared_exported_and_bound():
    import torch
    from rag import _native as nat
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crs_hip.h")).read(), flags=re.S)
    lib = nat.load()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, header), f"{name} not declared in include/crs_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in nat.exported_symbols(), f"{name} not in the binding table"
    assert lib.crs_abi_version() == 3
    for name, val in (("CRS_SPACE_COSINE", 0), ("CRS_SPACE_IP", 1), ("CRS_SPACE_L2", 2)):
        assert re.search(r"#define %s %d\b" % (name, val), header)
    assert (nat.SPACE_COSINE, nat.SPACE_IP, nat.SPACE_L2) == (0, 1, 2)
    ops = nat.ops()
    for name in ("rows_norm_max", "slab_append_space", "slab_write_rows_space", "slab_rescale_space", "queries_to_space", "space_distances"):
        assert hasattr(ops, name), name
    assert "Tensor emb, int space, Tensor norm_scale" in str(torch.ops.crs.slab_append_space.default._schema)
    for dim in (1, 100, 384, 1023):
        for space in (0, 1, 2):
            assert lib.crs_space_row_dim(dim, space) == nat.space_row_dim(dim, space) == dim + (space == 2)
    assert lib.crs_space_row_dim(0, 1) == 0 and lib.crs_space_row_dim(8, 3) == 0
    assert [nat.norm_scale_for(v) for v in (0.0, 0.3, 1.0, 1.5, 2.0, 5.0)] == [1.0, 0.5, 1.0, 2.0, 2.0, 8.0]


def test_argument_validation_without_gpu():
    from rag import _native as nat
    lib = nat.load()
    buf = (ctypes.c_char * 4096)()                     # host memory standing in for device pointers: never dereferenced
    p = ctypes.cast(buf, ctypes.c_void_p)
    EINVAL = -1
    # append(emb, n, dim, space, slab_type, norm_scale, slab, scales, shadow, row0, row_err, stream)
    for n, dim, space, st in ((1, 8, 0, 0), (1, 8, 3, 0), (1, 0, 1, 0), (1, 1025, 1, 0), (1, 1024, 2, 0), (-1, 8, 1, 0), (1, 8, 1, 2)):
        assert lib.crs_slab_append_space_f32(p, n, dim, space, st, p, p, p, p, 0, p, None) == EINVAL, (n, dim, space, st)
        assert lib.crs_slab_write_rows_space_f32(p, p, n, dim, space, st, p, p, p, p, 4, p, None) == EINVAL, (n, dim, space, st)
    assert lib.crs_slab_append_space_f32(p, 1, 8, 1, 1, p, p, None, p, 0, p, None) == EINVAL and b"int8 slab needs scales" in lib.crs_last_error()
    assert lib.crs_slab_append_space_f32(p, 1, 8, 1, 0, None, p, None, p, 0, p, None) == EINVAL and b"null pointer" in lib.crs_last_error()
    # rescale(n_rows, dim, space, slab_type, shift, slab, scales, shadow, row_err, stream)
    assert lib.crs_slab_rescale_space(4, 8, 1, 0, -1, p, None, p, p, None) == EINVAL and b"shift" in lib.crs_last_error()
    assert lib.crs_slab_rescale_space(4, 8, 1, 0, 127, p, None, p, p, None) == EINVAL
    assert lib.crs_slab_rescale_space(4, 8, 1, 0, 1, p, None, None, p, None) == EINVAL and b"shadow" in lib.crs_last_error()
    assert lib.crs_slab_rescale_space(4, 8, 1, 0, 0, p, None, p, p, None) == 0         # nothing to do: no launch
    # queries_to_space(q, nq, dim, space, slab_type, norm_scale, q32, q16, stream)
    assert lib.crs_queries_to_space(p, 1, 1024, 2, 0, p, p, p, None) == EINVAL
    assert lib.crs_queries_to_space(p, 1, 8, 1, 0, p, None, p, None) == EINVAL and b"null pointer" in lib.crs_last_error()
    # space_distances(q, nq, dim, space, shadow, n_rows, id_base, norm_scale, ids, k, out_dist, out_ids, stream)
    q = ctypes.cast((ctypes.c_char * 64)(), ctypes.c_void_p)
    for k in (0, 1025):
        assert lib.crs_space_distances(p, 1, 8, 1, p, 4, 0, p, p, k, p, q, None) == EINVAL and b"CRS_MAX_K_CERT" in lib.crs_last_error()
    assert lib.crs_space_distances(p, 1, 8, 1, p, 4, 0, p, p, 4, p, p, None) == EINVAL and b"must not be ids" in lib.crs_last_error()
    assert lib.crs_rows_norm_max(p, 1, 0, p, None, None) == EINVAL


class _Col:
    def __init__(self, space):
        self.metadata = {"hnsw:space": space}


class _Store:
    def __init__(self, space, with_collection=True):
        self.space = space
        self.collection = _Col(space) if with_collection else None


class _Model:
    has_normalize_module = None


@pytest.mark.parametrize("with_collection", [True, False])
def test_retriever_takes_the_ip_and_l2_branches(with_collection):
    from rag.retrieval import ContextRetriever
    ip = ContextRetriever(_Store("ip", with_collection), _Model(), {})
    assert ip.distance_metric == "ip"
    assert [ip._distance_to_similarity(v) for v in (-3.0, -1.0, 0.0, 1.0)] == [0.0, 0.5, 1.0, 1.0]
    l2 = ContextRetriever(_Store("l2", with_collection), _Model(), {})
    assert l2.distance_metric == "l2"
    assert [l2._distance_to_similarity(v) for v in (0.0, 1.0, 3.0)] == [1.0, 0.5, 0.25]
    cos = ContextRetriever(_Store("cosine", with_collection), _Model(), {})
    assert cos.distance_metric == "cosine" and cos._distance_to_similarity(1.0) == 0.5
    chunks = ip._hits_to_chunks(["a", "b"], ["ta", "tb"], None, [-1.0, 0.5])
    assert [c["score"] for c in chunks] == [0.5, 1.0] and [c["distance"] for c in chunks] == [-1.0, 0.5]


def test_store_distances_follow_the_space():
    from rag.indexing import VectorStore
    sc = np.array([0.75, -0.5], dtype=np.float32)
    assert VectorStore({}).distances_of(sc).tolist() == [0.25, 1.5]
    assert VectorStore({"space": "ip"}).distances_of(sc).tolist() == [0.75, -0.5]
    assert VectorStore({"space": "l2"}).distances_of(sc).dtype == np.float64


def test_warning_for_a_dot_product_model_on_a_cosine_store(caplog):
    from rag.retrieval import ContextRetriever

    class Dot(_Model):
        has_normalize_module = False

    class Unit(_Model):
        has_normalize_module = True

    def warnings_of(store, model):
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="rag.retrieval"):
            ContextRetriever(store, model, {})
        return [r for r in caplog.records if "Normalize" in r.getMessage()]

    assert len(warnings_of(_Store("cosine"), Dot())) == 1
    assert warnings_of(_Store("ip"), Dot()) == []
    assert warnings_of(_Store("cosine"), Unit()) == []
    assert warnings_of(_Store("cosine"), _Model()) == []          # synthetic weights: no modules.json to read
