"""CPU: the in-place mutation surface (delete / update / upsert) as far as it exists without a GPU.

  * the new C entry points are declared in include/crs_hip.h, exported by the library and bound in rag/_native.py; the two
    custom ops carry the documented schemas; argument validation answers -1 with a message before any HIP call; the ABI
    version is still 3 (the additions are additive);
  * the host arithmetic of the compaction (rows per window, windows walked, source row of every destination row, sidecar-row
    renumbering) against a numpy restatement over random dead sets, the edge cases included;
  * VectorStore.delete / update / upsert exist, SlabCollection mirrors them, and the argument errors that precede any device
    work are ValueErrors."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("crs_slab_write_rows_f32", "crs_slab_compact", "crs_slab_compact_bounce_bytes", "crs_slab_compact_window_rows")


def test_symbols_declared_exported_and_bound():
    from rag import _native as nat
    header = open(os.path.join(ROOT, "include", "crs_hip.h")).read()
    lib = nat.load()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in nat.exported_symbols()
        assert getattr(lib, name) is not None
    assert lib.crs_abi_version() == 3


def test_ops_registered_with_the_documented_schemas():
    import torch
    from rag import _native as nat
    nat.ops()
    assert str(torch.ops.crs.slab_compact.default._schema) == (
        "crs::slab_compact(Tensor dead, int n_rows, Tensor(a!) slab, Tensor(b!)? scales, Tensor(c!)? shadow, "
        "Tensor(d!)? rows_global, Tensor(e!) bounce, int first_row=0) -> ()")
    assert str(torch.ops.crs.slab_write_rows.default._schema) == (
        "crs::slab_write_rows(Tensor emb, Tensor rows, Tensor(a!) slab, Tensor(b!)? scales, Tensor(c!)? shadow, int n_rows, "
        "Tensor(d!)? row_err=None) -> ()")


def test_argument_validation_never_reaches_hip():
    """Every call below is refused by the argument checks: -1 (CRS_EINVAL) and a message.  The pointers are small fake
    addresses; a call that got past the checks would have to launch on them."""
    from rag import _native as nat
    lib = nat.load()
    p = ctypes.c_void_p
    fake, null = p(256), p(0)

    def msg():
        return lib.crs_last_error().decode()

    # crs_slab_compact(dead, m, n_rows, first_row, dim, slab_type, slab, scales, shadow, rows_global, bounce, bounce_bytes, stream)
    big = 1 << 28
    assert lib.crs_slab_compact(fake, -1, 10, 0, 384, 0, fake, null, null, null, fake, big, null) == -1 and "bad" in msg()
    assert lib.crs_slab_compact(fake, 11, 10, 0, 384, 0, fake, null, null, null, fake, big, null) == -1
    assert lib.crs_slab_compact(fake, 1, 10, 0, 0, 0, fake, null, null, null, fake, big, null) == -1
    assert lib.crs_slab_compact(fake, 1, 10, 0, 384, 7, fake, null, null, null, fake, big, null) == -1 and "slab_type" in msg()
    assert lib.crs_slab_compact(null, 1, 10, 0, 384, 0, fake, null, null, null, fake, big, null) == -1 and "null" in msg()
    assert lib.crs_slab_compact(fake, 1, 10, 0, 384, 0, null, null, null, null, fake, big, null) == -1 and "null" in msg()
    assert lib.crs_slab_compact(fake, 1, 10, 0, 384, 0, fake, null, null, null, null, big, null) == -1 and "null" in msg()
    assert lib.crs_slab_compact(fake, 1, 10, 0, 384, 0, fake, null, null, null, p(264), big, null) == -1 and "aligned" in msg()
    least = lib.crs_slab_compact_bounce_bytes(384, 0, 1)
    assert lib.crs_slab_compact(fake, 1, 10, 0, 384, 0, fake, null, fake, null, fake, least - 1, null) == -1 and "too small" in msg()
    # nothing to remove / nothing left: success without a launch, whatever the pointers
    assert lib.crs_slab_compact(null, 0, 10, 0, 384, 0, null, null, null, null, null, 0, null) == 0
    assert lib.crs_slab_compact(null, 10, 10, 0, 384, 0, null, null, null, null, null, 0, null) == 0
    # crs_slab_write_rows_f32(emb, rows, m, dim, slab_type, slab, scales, shadow, n_rows, row_err, stream)
    assert lib.crs_slab_write_rows_f32(fake, fake, -1, 384, 0, fake, null, null, 10, null, null) == -1
    assert lib.crs_slab_write_rows_f32(fake, fake, 1, 2000, 0, fake, null, null, 10, null, null) == -1
    assert lib.crs_slab_write_rows_f32(fake, fake, 1, 384, 3, fake, null, null, 10, null, null) == -1 and "slab_type" in msg()
    assert lib.crs_slab_write_rows_f32(null, fake, 1, 384, 0, fake, null, null, 10, null, null) == -1 and "null" in msg()
    assert lib.crs_slab_write_rows_f32(fake, null, 1, 384, 0, fake, null, null, 10, null, null) == -1 and "null" in msg()
    assert lib.crs_slab_write_rows_f32(fake, fake, 1, 384, 1, fake, null, null, 10, null, null) == -1 and "scales" in msg()
    assert lib.crs_slab_write_rows_f32(null, null, 0, 384, 0, null, null, null, 10, null, null) == 0
    assert lib.crs_slab_compact_bounce_bytes(0, 0, 1) == 0 and lib.crs_slab_compact_bounce_bytes(384, 9, 1) == 0


@pytest.mark.parametrize("dim,st,shadow", [(384, 0, True), (384, 1, True), (100, 0, True), (101, 0, True), (1000, 1, False), (768, 0, False)])
def test_bounce_size_and_window_rows(dim, st, shadow):
    """The smallest legal bounce holds a window of exactly 1024 rows of every array; one byte less holds none; windows are
    whole workgroups (32 rows); the default size is min(256 MB, the whole shard) and never below the minimum."""
    from rag import _native as nat
    row = nat.padded_dim(dim, st) * (1 if st else 2) + (4 * dim if shadow else 0) + 4 + 8
    least = nat.slab_compact_bounce_bytes(dim, st, shadow)
    assert 1024 * row <= least <= 1024 * row + 2048
    assert nat.slab_compact_window_rows(dim, st, shadow, least) == 1024
    assert nat.slab_compact_window_rows(dim, st, shadow, least - 1) == 0
    for size in (least + 1, 3 * least + 77, 256 << 20):
        w = nat.slab_compact_window_rows(dim, st, shadow, size)
        assert w >= 1024 and w % 32 == 0 and w * row <= size and (w + 32) * row + 2048 > size
    assert nat.compact_bounce_size(10, dim, st, shadow) == least
    assert nat.compact_bounce_size(100_000_000, dim, st, shadow) == 256 << 20
    mid = nat.compact_bounce_size(100_003, dim, st, shadow)
    assert least <= mid <= 256 << 20 and nat.slab_compact_window_rows(dim, st, shadow, mid) >= min(100_003, (256 << 20) // row - 64)


def _dead_sets(n, w, rng):
    yield "none", np.zeros(0, dtype=np.int64)
    yield "all", np.arange(n, dtype=np.int64)
    yield "first", np.array([0], dtype=np.int64)
    yield "last", np.array([n - 1], dtype=np.int64)
    yield "middle", np.array([n // 2], dtype=np.int64)
    yield "every other", np.arange(0, n, 2, dtype=np.int64)
    yield "block longer than a window", np.arange(n // 3, n // 3 + w + 17, dtype=np.int64)
    for frac in (0.01, 0.5, 0.99):
        yield f"random {frac}", np.sort(rng.choice(n, max(1, int(n * frac)), replace=False)).astype(np.int64)


def test_planning_against_numpy():
    """source(d) = d + #{i : dead[i] - i <= d} (the kernel's rule, restated with searchsorted) equals the survivors in order;
    the windows cover exactly the destinations at or above the window of the first dead row, in order, without overlap;
    every window reads only rows at or above its own first row (the ordering argument of csrc/mutate.hip)."""
    from rag.indexing import compact_windows, renumber_rows, survivor_rows
    rng = np.random.default_rng(5)
    n, w = 5000, 1024
    for name, dead in _dead_sets(n, w, rng):
        src = survivor_rows(n, dead)
        m = len(dead)
        assert len(src) == n - m, name
        d = np.arange(n - m, dtype=np.int64)
        rule = d + np.searchsorted(dead - np.arange(m), d, side="right")       # j = #{dead[i] - i <= d}
        assert np.array_equal(rule, src), name
        first = int(dead[0]) if m else 0
        wins = compact_windows(n, m, w, first)
        if m == 0 or m == n:
            assert wins == [], name
            continue
        assert wins[0][0] == first // w * w and wins[0][0] <= first, name
        assert all(a[0] + a[1] == b[0] for a, b in zip(wins, wins[1:])) and wins[-1][0] + wins[-1][1] == n - m, name
        assert all(0 < ww <= w for _, ww in wins), name
        for d0, ww in wins:
            assert src[d0: d0 + ww].min() >= d0, name                            # sources never lie below the window
        assert np.array_equal(src[:first], np.arange(first)), name               # rows below dead[0] do not move
        # sidecar renumbering: the survivors' new rows are 0, 1, 2, ...
        assert np.array_equal(renumber_rows(src, dead), np.arange(n - m)), name
        assert compact_windows(n, m, w, 0)[-len(wins):] == wins, name            # the hint only drops leading windows


def test_store_methods_exist_and_refuse_bad_arguments_without_a_gpu():
    from rag.indexing import SlabCollection, VectorStore
    from rag.pipeline import RAGPipeline
    store = VectorStore({})
    assert store.mutation_epoch == 0
    for name in ("delete", "update", "upsert"):
        assert callable(getattr(store, name)) and callable(getattr(SlabCollection, name))
    assert callable(RAGPipeline.remove_documents)
    with pytest.raises(ValueError, match="needs ids, where or where_document"):
        store.delete()
    with pytest.raises(ValueError, match="needs ids, where or where_document"):
        store.delete(ids=None, where={}, where_document=None)
    with pytest.raises(ValueError, match="No collection available"):
        store.delete(ids=["a"])
    with pytest.raises(ValueError, match="No collection available"):
        store.update(["a"], documents=["x"])
    with pytest.raises(ValueError, match="doesn't match embedding count"):
        store.upsert([object()], np.zeros((2, 8), dtype=np.float32))
    assert store.mutation_epoch == 0

    # a collection assembled on the host (one EMPTY shard on the cpu device, so nothing is launched): every check of update()
    # precedes device work, and sidecar-only changes need none
    import torch
    col = SlabCollection("t", "fp16", True, [torch.device("cpu")])
    col.shards[0].dim, col.shards[0].pdim = 8, 128
    col.ids, col.documents, col.metadatas = ["a", "b", "b", "c"], ["A", "B", "B2", "C"], [{}, {}, {}, {"k": 1}]
    store.collection = store._adopt(col)
    with pytest.raises(ValueError, match="unknown id"):
        store.update(["zzz"], documents=["x"])
    with pytest.raises(ValueError, match="carried by 2 rows"):
        store.update(["b"], documents=["x"])
    with pytest.raises(ValueError, match="given twice"):
        store.update(["a", "a"], documents=["x", "y"])
    with pytest.raises(ValueError, match="documents count"):
        store.update(["a", "c"], documents=["x"])
    with pytest.raises(ValueError, match="metadatas count"):
        store.update(["a"], metadatas=[{}, {}])
    with pytest.raises(ValueError, match="Embedding dimension 5"):
        store.update(["a"], embeddings=np.zeros((1, 5), dtype=np.float32))
    with pytest.raises(ValueError, match="2-D"):
        store.update(["a"], embeddings=np.zeros((1, 2, 4), dtype=np.float32))
    assert col.documents == ["A", "B", "B2", "C"] and store.mutation_epoch == 0
    # texts and metadata, the dict replaced whole; the collection's delegates reach the store
    col.update(["c"], documents=["C2"], metadatas=[{"j": 2}])
    assert col.documents[3] == "C2" and col.metadatas[3] == {"j": 2} and store.mutation_epoch == 1
    assert store.delete(ids=["nobody"]) == 0 and store.delete(ids=[]) == 0 and store.mutation_epoch == 1
    assert store.delete(ids=["a"], where={"j": 2}) == 0            # AND of the two parts
    assert store.delete(where={"j": 2}) == 1 and col.ids == ["a", "b", "b"] and store.mutation_epoch == 2
    assert col.delete(ids=["b", "ghost"]) == 2 and col.ids == ["a"] and col.count() == 1
    assert col._id_rows() == {"a": [0]}
