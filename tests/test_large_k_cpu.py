"""No GPU: the partition behind the certified top_k 65..1024 search (nat.large_k_plan, crs_large_k_plan) and the argument
checks of its C entries.

The plan cuts a shard into chunks that are scanned for 64 candidates each: the chunks must cover every row exactly once, be
whole multiples of 16 rows (all but the last), and keep parts x 64 <= 4096 candidates per query (the LDS list of the re-rank
kernel, csrc/large_k.hip)."""
import ctypes

import numpy as np
import pytest

SIZES = sorted({1, 2, 15, 16, 17, 31, 63, 64, 65, 100, 127, 128, 129, 1000, 1023, 1024, 1025, 4095, 4096, 4097, 65_535,
                300_000, 1_000_003, 10_000_000, 100_000_000} | set(np.unique(np.logspace(0, 8, 60).astype(np.int64)).tolist()))
KS = list(range(1, 130)) + [200, 255, 256, 257, 500, 511, 512, 513, 999, 1000, 1008, 1009, 1023, 1024]


def test_plan_covers_every_row_once_in_whole_groups_of_16():
    from rag import _native as nat
    for k in KS:
        want = min(64, max(2, -(-k // 16)))
        for n in SIZES:
            parts, rows = nat.large_k_plan(k, n)
            assert rows % 16 == 0 and rows > 0, (k, n, rows)
            assert 1 <= parts <= want and parts * 64 <= 4096, (k, n, parts)
            assert (parts - 1) * rows < n <= parts * rows, f"k {k} n {n}: {parts} x {rows} rows do not cover the shard exactly"
            if n > 16 * want * (want - 1):          # large shards get every chunk asked for
                assert parts == want, (k, n, parts, want)
            # row r belongs to exactly one chunk: r // rows
            last = n - (parts - 1) * rows
            assert 0 < last <= rows


def test_plan_depth_covers_top_k():
    """Each chunk's 64-deep list is at least 4 x its even share of the top-k_out (k_out / P <= 16) on large shards."""
    from rag import _native as nat
    for k in range(65, nat.MAX_K_CERT + 1):
        parts, _ = nat.large_k_plan(k, 10_000_000)
        assert k / parts <= 16, (k, parts)
        assert parts * 64 >= k


def test_plan_and_candidate_bytes_agree_with_the_library():
    from rag import _native as nat
    lib = nat.load()
    assert nat.MAX_K_CERT == 1024
    for nq in (1, 7, 64, 300):
        for k in (1, 64, 65, 100, 256, 1000, 1024):
            for n in (1, 17, 64, 1000, 4097, 300_000, 10_000_000, 100_000_000):
                p, r, b = ctypes.c_int(), ctypes.c_int64(), ctypes.c_size_t()
                assert lib.crs_large_k_plan(nq, k, n, ctypes.byref(p), ctypes.byref(r), ctypes.byref(b)) == 0
                assert (p.value, r.value) == nat.large_k_plan(k, n), (nq, k, n)
                assert b.value == nat.large_k_cand_bytes(nq, k, n), (nq, k, n)
                slots = p.value * nq * 64
                assert b.value >= slots * 12 and b.value % 256 == 0


def test_large_k_argument_validation_without_gpu():
    from rag import _native as nat
    lib = nat.load()
    p, r, b = ctypes.c_int(), ctypes.c_int64(), ctypes.c_size_t()
    assert lib.crs_large_k_plan(4, 1025, 1000, ctypes.byref(p), ctypes.byref(r), ctypes.byref(b)) == -1
    assert b"CRS_MAX_K_CERT" in lib.crs_last_error()
    assert lib.crs_large_k_plan(4, 0, 1000, ctypes.byref(p), ctypes.byref(r), ctypes.byref(b)) == -1
    assert lib.crs_large_k_plan(0, 100, 1000, ctypes.byref(p), ctypes.byref(r), ctypes.byref(b)) == -1
    assert lib.crs_large_k_plan(4, 100, 0, ctypes.byref(p), ctypes.byref(r), ctypes.byref(b)) == -1
    assert lib.crs_large_k_plan(4, 100, 1000, None, ctypes.byref(r), ctypes.byref(b)) == -1
    out = ctypes.c_size_t(0)
    assert lib.crs_cosine_topk_large_cert_workspace_bytes(4, 384, 2000, 1000, ctypes.byref(out)) == -1
    # the kernel entry refuses a partition that does not cover n_rows, or one with an empty chunk, before any HIP call
    ws_bytes = nat.exact_workspace_bytes(4, 4096)
    fake = ctypes.c_void_p(256)
    args = lambda parts, rows, k: (fake, fake, 4, 384, 0, fake, 1000, 0, fake, fake, parts, rows, k, 0.0, fake, fake, fake, fake,  # noqa: E731
                                   ws_bytes, 4096, None)
    assert lib.crs_refine_large_cert(*args(2, 496, 100)) == -1                  # 992 < 1000 rows
    assert lib.crs_refine_large_cert(*args(3, 500, 100)) == -1                  # the third chunk would be empty
    assert lib.crs_refine_large_cert(*args(65, 16, 100)) == -1                  # more than 64 chunks
    assert lib.crs_refine_large_cert(*args(2, 512, 1025)) == -1                 # k_out above CRS_MAX_K_CERT
    assert lib.crs_cosine_topk_large_cert(fake, 4, 384, 5, fake, None, 1000, 0, fake, 1 << 30, fake, fake, 100, 0.0, fake, fake, fake,
                                          fake, ws_bytes, 4096, None) == -1      # bad slab type
    # escalation: k_out above 64 needs a list of at least k_out rows; above CRS_MAX_K_CERT it is refused
    esc = lambda k, cap: lib.crs_escalate_exact(fake, fake, 4, 384, 0, fake, None, fake, 1000, 0, k, fake, fake, fake, fake,  # noqa: E731
                                                nat.exact_workspace_bytes(4, cap), cap, None)
    assert esc(100, 64) == -1 and b"cap >= k_out" in lib.crs_last_error()
    assert esc(1025, 4096) == -1


@pytest.mark.parametrize("k", [65, 1024])
def test_store_routes_top_k_to_the_certified_path_up_to_max_k_cert(k):
    """The escalation list of a large top_k starts at 4 x top_k rows (>= exact_cap), never above EXACT_MAX_CAP."""
    from rag import _native as nat
    from rag.indexing import VectorStore
    vs = VectorStore.__new__(VectorStore)
    vs.exact_cap = nat.EXACT_CAP
    assert vs._cap(10) == nat.EXACT_CAP and vs._cap(64) == nat.EXACT_CAP
    assert vs._cap(k) == min(nat.EXACT_MAX_CAP, max(nat.EXACT_CAP, 4 * k)) >= k
