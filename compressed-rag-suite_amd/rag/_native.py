"""Bindings of the native library.

Compute calls go through the PyTorch-ROCm custom ops ``torch.ops.crs.*`` that csrc/torch_ops.cpp registers with
TORCH_LIBRARY (libcrs_torch.so; tensors in, current HIP stream) over the C ABI of libcrs_hip.so
(include/crs_hip.h, include/crs_encoder.h).  The C ABI itself is bound with ctypes for the host-side
queries (row padding, workspace sizes, plan description, the timing hook) and stays the drop-in boundary for
non-torch hosts.  There is no CPU fallback anywhere in this module: if a shared library is
missing, or there is no GPU, the calls raise.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_int64, c_size_t, c_void_p, POINTER, byref

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CRS_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "csrc", "libcrs_hip.so")  # override: A/B builds
TORCH_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libcrs_torch.so")

SLAB_F16 = 0
SLAB_I8 = 1
MAX_K = 64
MAX_K_CERT = 1024          # CRS_MAX_K_CERT: largest top_k with a certificate (partitioned over-fetch, csrc/large_k.hip)
MERGE_SORTED_MAX_LISTS = 64   # crs_merge_sorted: lists per query (csrc/merge_sorted.hip)
LARGE_K_MAX_PARTS = 64     # chunks of the partition (x 64 candidates: at most 4096 per query)
EXACT_MAX_CAP = 13312      # CRS_EXACT_MAX_CAP: longest per-query row list of crs_escalate_exact
EXACT_CAP = 1024           # default list length (12 KB of LDS per query in the re-rank)
BM25_MAX_QUERIES = 64      # queries of one crs_bm25_topk launch
WORDPIECE_TILE_BYTES = 1024   # CRS_WORDPIECE_TILE_BYTES: bytes of a text that crs_wordpiece_encode stages at a time
UNIGRAM_TILE_BYTES = 1024     # CRS_UNIGRAM_TILE_BYTES: the same for crs_unigram_encode
UNIGRAM_MAX_WORD = 128        # CRS_UNIGRAM_MAX_WORD: code points of the longest word it walks (U+2581 included); longer: the host's
UNIGRAM_COLLAPSE, UNIGRAM_SINGLE_META, UNIGRAM_RUN_META, UNIGRAM_CRLF = 1, 2, 4, 8    # CRS_UNIGRAM_* option bits
BM25_MAX_PAIRS = 4096      # CRS_BM25_MAX_PAIRS: (query, known token) pairs of one crs_bm25_topk launch
SPARSE_MAX_TERMS = 1024    # CRS_SPARSE_MAX_TERMS: terms of one text after crs_sparse_compact (csrc/sparse_compact.hip)
SPARSE_MAX_SKIP = 16       # CRS_SPARSE_MAX_SKIP: ids crs_sparse_compact always drops
MAXSIM_MAX_QUERY = 64      # CRS_MAXSIM_MAX_QUERY: query tokens of crs_maxsim (csrc/maxsim.hip)
PAIRS_TILE = 256           # CRS_PAIRS_TILE: tile edge of the near-duplicate join (csrc/join.hip)
PAIRS_MAX_TILES = 1 << 22  # CRS_PAIRS_MAX_TILES: tile pairs of one crs_pairs_above_f16 launch
SPACE_COSINE, SPACE_IP, SPACE_L2 = 0, 1, 2    # CRS_SPACE_*: a collection's hnsw:space
SPACES = {"cosine": SPACE_COSINE, "ip": SPACE_IP, "l2": SPACE_L2}

class MlmPlan(ctypes.Structure):
    """crs_mlm_plan (include/crs_encoder.h): the launch geometry of crs_mlm_sparse_pool."""
    _fields_ = [(n, ctypes.c_int32) for n in (
        "tile_m", "tile_n", "tile_k", "tokens", "tokens_padded", "grid_m", "grid_n", "pool_grid", "pool_threads", "pool_lds_bytes",
        "xform_grid", "xform_threads", "xform_lds_bytes", "ew_grid_x", "ew_threads")] + [("t16_bytes", c_size_t), ("workspace_bytes", c_size_t)]


# name -> (restype, argtypes); mirrors include/crs_hip.h one to one
_SIGNATURES = {
    "crs_last_error": (c_char_p, []),
    "crs_abi_version": (c_int, []),
    "crs_padded_dim": (c_int, [c_int]),
    "crs_row_elems": (c_int, [c_int, c_int]),
    "crs_slab_append_f32": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                    c_int64, c_void_p, c_void_p]),
    "crs_slab_write_rows_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                        c_void_p]),
    "crs_slab_compact_bounce_bytes": (c_size_t, [c_int, c_int, c_int]),
    "crs_slab_compact_window_rows": (c_int64, [c_int, c_int, c_int, c_size_t]),
    "crs_slab_compact": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_size_t, c_void_p]),
    "crs_queries_to_f16": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "crs_space_row_dim": (c_int, [c_int, c_int]),
    "crs_rows_norm_max": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "crs_slab_append_space_f32": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                          c_void_p, c_void_p]),
    "crs_slab_write_rows_space_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_int64, c_void_p, c_void_p]),
    "crs_slab_rescale_space": (c_int, [c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "crs_queries_to_space": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "crs_space_distances": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int, c_void_p,
                                    c_void_p, c_void_p]),
    "crs_scan_workspace_bytes": (c_int, [c_int, c_int, c_int, c_int64, POINTER(c_size_t)]),
    "crs_cosine_topk": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int64, c_int,
                                c_int64, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "crs_merge_topk": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                               c_void_p]),
    "crs_merge_sorted": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "crs_mmr_order": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.c_double, c_void_p, c_void_p]),
    "crs_token_match": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "crs_rerank_lexical": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64,
                                   c_void_p, c_int, ctypes.c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "crs_token_project": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p]),
    "crs_maxsim": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int, c_int, c_void_p,
                           c_void_p]),
    "crs_pairs_above_f16": (c_int, [c_void_p, c_int64, c_int, c_int64, c_int64, c_int64, c_int64, c_float, c_void_p, c_void_p, c_int64,
                                    c_void_p, c_void_p]),
    "crs_pairs_verify_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "crs_bm25_workspace_bytes": (c_int, [c_int, c_int, c_int64, POINTER(c_size_t)]),
    "crs_bm25_topk": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_int64,
                              c_float, c_float, c_float, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "crs_sparse_compact": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "crs_sparse_workspace_bytes": (c_int, [c_int, c_int, c_int64, POINTER(c_size_t)]),
    "crs_sparse_topk": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p,
                                c_size_t, c_void_p, c_void_p, c_void_p]),
    "crs_mlm_pool_plan": (c_int, [c_int, c_int, c_int, c_int, POINTER(MlmPlan)]),
    "crs_mlm_workspace_bytes": (c_int, [c_int, c_int, c_int, c_int, POINTER(c_size_t)]),
    "crs_mlm_sparse_pool": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_int, c_void_p]),
    "crs_fuse_rrf": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_int, c_void_p,
                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "crs_wordpiece_encode": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                                     c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                     c_void_p, c_void_p]),
    "crs_unigram_encode": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                   c_void_p, c_int64, c_int, c_int, ctypes.c_double, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                   c_void_p, c_void_p, c_void_p]),
    "crs_encoder_plan_describe": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t]),   # crs_encoder_desc by pointer
    "crs_rescore_f32": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int64, c_int64, c_int, c_void_p,
                                c_void_p, c_void_p]),
    "crs_score_rows_f32": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "crs_refine_f32": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int64, c_int64, c_void_p, c_int, c_int,
                               c_void_p, c_void_p, c_void_p]),
    "crs_exact_workspace_bytes": (c_size_t, [c_int, c_int]),
    "crs_exact_row_error_bound": (c_float, [c_int, c_int]),
    "crs_refine_f32_cert": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int64, c_int64, c_void_p, c_void_p,
                                    c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    "crs_cosine_topk_cert": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int64, c_int, c_int64, c_void_p, c_size_t,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_size_t, c_int, c_void_p]),
    "crs_escalate_exact": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                   c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    "crs_large_k_plan": (c_int, [c_int, c_int, c_int64, POINTER(c_int), POINTER(c_int64), POINTER(c_size_t)]),
    "crs_cosine_topk_large_cert_workspace_bytes": (c_int, [c_int, c_int, c_int, c_int64, POINTER(c_size_t)]),
    "crs_cosine_topk_large_cert": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_size_t,
                                           c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int,
                                           c_void_p]),
    "crs_refine_large_cert": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int,
                                      c_int64, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    "crs_wire_bytes": (c_size_t, [c_int, c_int]),
    "crs_wire_scores_offset": (c_size_t, [c_int, c_int]),
    "crs_merge_topk_wire": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "crs_merge_sorted_wire": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "crs_scan_plan_describe": (c_int, [c_int, c_int, c_int, c_int64, c_int, ctypes.c_char_p, c_size_t]),
    "crs_stream_create_cu_masked": (c_int, [c_int, c_int, POINTER(c_void_p)]),
    "crs_stream_destroy": (c_int, [c_void_p]),
    "crs_time_cosine_topk": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int64,
                                     c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_int,
                                     POINTER(c_float), POINTER(c_float)]),
}

_lib = None


class NativeError(RuntimeError):
    """A libcrs_hip.so call failed (the message comes from crs_last_error())."""


def register_signatures(table: dict) -> None:
    """Let sibling modules (the encoder binding) add their entry points before load()."""
    _SIGNATURES.update(table)
    if _lib is not None:
        for name, (res, args) in table.items():
            fn = getattr(_lib, name)
            fn.restype, fn.argtypes = res, args


def load() -> ctypes.CDLL:
    """dlopen the in-tree library; raises loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"or `make -C {os.path.dirname(LIB_PATH)}` -- this path has no CPU fallback")
        # torch first: it ships its own HIP runtime and both must resolve to ONE libamdhip64 in the
        # process (loading ours first leaves the kernels on a runtime that sees no device)
        import torch  # noqa: F401
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError = header/library mismatch
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


_ops = None


def ops():
    """``torch.ops.crs`` -- the PyTorch custom ops of libcrs_torch.so (loaded once; raises when it has not been built)."""
    global _ops
    if _ops is None:
        load()                                  # the C-ABI library first (libcrs_torch.so links against it by file name)
        if not os.path.exists(TORCH_LIB_PATH):
            raise NativeError(f"{TORCH_LIB_PATH} is missing: build it with `make -C {os.path.dirname(TORCH_LIB_PATH)}` "
                              f"-- this path has no CPU fallback")
        import torch
        torch.ops.load_library(TORCH_LIB_PATH)
        _ops = torch.ops.crs
    return _ops


class _translate:
    """torch custom ops raise RuntimeError (TORCH_CHECK); the callers of this module catch NativeError."""
    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        if et is not None and issubclass(et, RuntimeError) and not issubclass(et, NativeError):
            raise NativeError(str(ev).split("\n")[0]) from ev
        return False


def exported_symbols():
    return sorted(_SIGNATURES)


def check(rc: int) -> None:
    if rc != 0:
        msg = load().crs_last_error()
        raise NativeError(f"libcrs_hip error {rc}: {msg.decode() if msg else '?'}")


def padded_dim(dim: int, slab_type: int = SLAB_F16) -> int:
    """Padded row length of a slab (and of the queries searched against it)."""
    return int(load().crs_row_elems(int(dim), int(slab_type)))


def _stream_ptr():
    import torch
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise NativeError("no ROCm GPU visible: the MI355X vector store has no CPU fallback")


# ----------------------------------------------------------------------------- wrappers
def slab_append_f32(emb, slab, row0: int, slab_type: int, scales=None, shadow=None, row_err=None) -> None:
    """emb: cuda fp32 [n, dim]; slab: cuda fp16/int8 [cap, pdim]; writes rows row0..row0+n.
    row_err: cuda fp32 [1] (zeroed by the owner of the slab) raised to the largest |stored row - fp32 row|_2."""
    if emb.shape[0] == 0:
        return
    with _translate():
        ops().slab_append(emb, slab, scales, shadow, int(row0), row_err)


def slab_write_rows_f32(emb, rows, slab, n_rows: int, scales=None, shadow=None, row_err=None) -> None:
    """The scatter form of slab_append_f32: emb cuda fp32 [m, dim] -> rows `rows` (cuda int64 [m], distinct, < n_rows) of slab /
    scales / shadow, through the same per-row device function as the append (same bits); row_err raised likewise."""
    if emb.shape[0] == 0:
        return
    with _translate():
        ops().slab_write_rows(emb, rows, slab, scales, shadow, int(n_rows), row_err)


COMPACT_BOUNCE_MAX = 256 << 20     # the bounce buffer VectorStore.delete allocates at most (and frees after the call)


def slab_compact_bounce_bytes(dim: int, slab_type: int, has_shadow: bool) -> int:
    """Smallest legal bounce buffer of slab_compact: one window of 1024 rows of every array."""
    return int(load().crs_slab_compact_bounce_bytes(int(dim), int(slab_type), int(bool(has_shadow))))


def slab_compact_window_rows(dim: int, slab_type: int, has_shadow: bool, bounce_bytes: int) -> int:
    """Rows per window of slab_compact for a bounce size (0: too small)."""
    return int(load().crs_slab_compact_window_rows(int(dim), int(slab_type), int(bool(has_shadow)), int(bounce_bytes)))


def compact_bounce_size(n_rows: int, dim: int, slab_type: int, has_shadow: bool) -> int:
    """min(COMPACT_BOUNCE_MAX, one window over all n_rows rows), never below the legal minimum.  Host arithmetic."""
    least = slab_compact_bounce_bytes(dim, slab_type, has_shadow)
    per_row = (least - 4 * 256 - 16) // 1024
    whole = (-(-int(n_rows) // 32) * 32) * per_row + 4 * 256 + 16
    return max(least, min(COMPACT_BOUNCE_MAX, whole))


def slab_compact(dead, n_rows: int, slab, scales=None, shadow=None, rows_global=None, bounce=None, first_row: int = 0) -> None:
    """Remove the rows `dead` (cuda int64, strictly ascending, < n_rows) from slab / scales / shadow / rows_global in place,
    keeping the order of the others (crs_slab_compact): rows [0, n_rows - len(dead)) hold the survivors afterwards.  No
    allocation beside the bounce buffer (made here, and dropped on return, when none is passed); no host sync."""
    import torch
    if dead.numel() == 0:
        return
    if bounce is None:
        dim = shadow.shape[1] if shadow is not None else slab.shape[1]
        st = SLAB_I8 if slab.dtype == torch.int8 else SLAB_F16
        bounce = torch.empty(compact_bounce_size(n_rows, dim, st, shadow is not None), dtype=torch.uint8, device=slab.device)
    with _translate():
        ops().slab_compact(dead, int(n_rows), slab, scales, shadow, rows_global, bounce, int(first_row))


def queries_to_f16(q32, slab_type: int = SLAB_F16, out=None):
    import torch
    nq, dim = q32.shape
    if out is None:
        out = torch.empty((nq, padded_dim(dim, slab_type)), dtype=torch.float16, device=q32.device)
    if nq:
        with _translate():
            ops().queries_to_f16(q32, out, int(slab_type))
    return out


# ---- hnsw:space 'ip' / 'l2' (csrc/space.hip, csrc/row_build.hip; include/crs_hip.h holds the contracts, DESIGN 3.12 the transform)
def space_row_dim(dim: int, space: int) -> int:
    """d': the coordinates a stored row and a converted query have (dim, or dim + 1 for l2).  Host arithmetic, no library."""
    return int(dim) + (1 if int(space) == SPACE_L2 else 0)


def norm_scale_for(norm: float) -> float:
    """The smallest power of two >= norm (1.0 for a zero norm): the store's R for a largest row norm."""
    import math
    if not norm > 0.0:
        return 1.0
    m, e = math.frexp(float(norm))                 # norm = m 2^e, 0.5 <= m < 1
    return math.ldexp(1.0, e - 1 if m == 0.5 else e)


def covering_norm(norm_max: float, dim: int) -> float:
    """An upper bound of the TRUE largest norm behind rows_norm_max's fp32 result.  That norm is ceil(dim/64) fmas and six
    butterfly additions of non-negative terms and one square root: it can fall short of the true norm by the relative
    ((ceil(dim/64) + 7) / 2 + 1) 2^-24, and round down onto a power of two.  Inflating it by (ceil(dim/64) + 8) 2^-24
    -- more than that bound -- before it is mapped to R keeps every stored row's norm <= 1; a norm of exactly 2^e then gets
    R = 2^(e + 1), which is correct and harmless."""
    return float(norm_max) * (1.0 + (-(-int(dim) // 64) + 8) * 2.0 ** -24)


def rows_norm_max(emb) -> float:
    """The largest |x|_2 of emb (cuda fp32 [n, dim]) as a host float: one launch, one 4-byte readback; inf when a norm is not
    finite."""
    import torch
    if emb.shape[0] == 0:
        return 0.0
    out = torch.zeros(1, dtype=torch.float32, device=emb.device)
    with _translate():
        ops().rows_norm_max(emb, out)
    return float(out.item())


def slab_append_space_f32(emb, space: int, norm_scale, slab, row0: int, scales=None, shadow=None, row_err=None) -> None:
    """slab_append_f32 for a store of space ip / l2: emb cuda fp32 [n, dim] -> rows row0.. of slab [cap, padded d'], scales, shadow
    [cap, d'] under the scale norm_scale (cuda fp32 [1], a power of two >= every norm of emb).  Rows are not normalised."""
    if emb.shape[0] == 0:
        return
    with _translate():
        ops().slab_append_space(emb, int(space), norm_scale, slab, scales, shadow, int(row0), row_err)


def slab_write_rows_space_f32(emb, rows, space: int, norm_scale, slab, n_rows: int, scales=None, shadow=None, row_err=None) -> None:
    """The scatter form of slab_append_space_f32 (same per-row device function, same bits)."""
    if emb.shape[0] == 0:
        return
    with _translate():
        ops().slab_write_rows_space(emb, rows, int(space), norm_scale, slab, scales, shadow, int(n_rows), row_err)


def slab_rescale_space(n_rows: int, dim: int, space: int, shift: int, slab, shadow, scales=None, row_err=None) -> None:
    """The scale grew by 2^shift: rows [0, n_rows) of shadow are multiplied by 2^-shift (l2's last coordinate by 2^-2 shift) and the
    slab rows and int8 scales rebuilt from them, exactly.  dim is the caller's dimension.  One launch."""
    if n_rows <= 0 or shift <= 0:
        return
    with _translate():
        ops().slab_rescale_space(int(n_rows), int(dim), int(space), int(shift), slab, scales, shadow, row_err)


def queries_to_space(q, space: int, slab_type: int, norm_scale, out32=None, out16=None):
    """q cuda fp32 [nq, dim], any norm -> (unit fp32 [nq, d'], fp16 [nq, padded d']): the q32 / q16 of a certified search."""
    import torch
    nq, dim = q.shape
    sdim = space_row_dim(dim, space)
    if out32 is None:
        out32 = torch.empty((nq, sdim), dtype=torch.float32, device=q.device)
    if out16 is None:
        out16 = torch.empty((nq, padded_dim(sdim, slab_type)), dtype=torch.float16, device=q.device)
    if nq:
        with _translate():
            ops().queries_to_space(q, int(space), int(slab_type), norm_scale, out32, out16)
    return out32, out16


def space_distances(q, space: int, shadow, n_rows: int, id_base: int, norm_scale, ids):
    """The distances of finished lists: q cuda fp32 [nq, dim] (the caller's queries), ids int64 [nq, k <= MAX_K_CERT] (rows +
    id_base of the view whose shadow / n_rows are given) -> (distances fp32 [nq, k], ids [nq, k]) ordered (distance asc, id asc),
    empty slots (+inf, -1) last.  ip: 1 - <q, x>; l2: sum (q - x)^2, computed from the recovered vectors."""
    import torch
    out_d = torch.empty(ids.shape, dtype=torch.float32, device=q.device)
    out_i = torch.empty(ids.shape, dtype=torch.int64, device=q.device)
    with _translate():
        ops().space_distances(q, int(space), shadow, int(n_rows), int(id_base), norm_scale, ids.contiguous(), out_d, out_i)
    return out_d, out_i


def scan_workspace_bytes(nq: int, dim: int, k: int, n_rows: int) -> int:
    out = c_size_t(0)
    check(load().crs_scan_workspace_bytes(nq, dim, k, n_rows, byref(out)))
    return int(out.value)


def cosine_topk(q16, slab, n_rows: int, dim: int, k: int, *, slab_type: int = SLAB_F16, scales=None,
                id_base: int = 0, workspace=None, out_scores=None, out_ids=None):
    """q16: cuda fp16 [nq, pdim]; slab: cuda [>= n_rows, pdim]. Returns (scores fp32, ids int64) [nq, k]."""
    import torch
    nq = q16.shape[0]
    need = scan_workspace_bytes(nq, dim, k, n_rows)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=q16.device)
    if out_scores is None:
        out_scores = torch.empty((nq, k), dtype=torch.float32, device=q16.device)
    if out_ids is None:
        out_ids = torch.empty((nq, k), dtype=torch.int64, device=q16.device)
    with _translate():
        ops().cosine_topk_out(q16, slab, scales, int(n_rows), int(dim), int(k), int(id_base), workspace, out_scores, out_ids)
    return out_scores, out_ids


def merge_topk(scores, ids, k_out: int, out_scores=None, out_ids=None):
    """scores/ids: cuda [G, nq, k_in] (fp32 / int64) -> global top-k_out per query."""
    import torch
    g, nq, k_in = scores.shape
    out_s = out_scores if out_scores is not None else torch.empty((nq, k_out), dtype=torch.float32, device=scores.device)
    out_i = out_ids if out_ids is not None else torch.empty((nq, k_out), dtype=torch.int64, device=scores.device)
    with _translate():
        ops().merge_topk_out(scores, ids, int(k_out), out_s, out_i)
    return out_s, out_i


def merge_sorted(scores, ids, k_out: int, out_scores=None, out_ids=None):
    """merge_topk for k above MAX_K: scores/ids cuda [G, nq, k_in], every list ALREADY sorted (score desc, id asc, empty slots
    (-inf, -1) last), ids >= 0 distinct across lists -> the first k_out of their union, same bits, same order.
    G <= 64, k_in and k_out <= MAX_K_CERT (csrc/merge_sorted.hip)."""
    import torch
    g, nq, k_in = scores.shape
    out_s = out_scores if out_scores is not None else torch.empty((nq, k_out), dtype=torch.float32, device=scores.device)
    out_i = out_ids if out_ids is not None else torch.empty((nq, k_out), dtype=torch.int64, device=scores.device)
    with _translate():
        ops().merge_sorted_out(scores, ids, int(k_out), out_s, out_i)
    return out_s, out_i


def mmr_order(vecs, n_rows: int, rows, rel, counts, lam: float, out=None):
    """Greedy MMR order of nq lists of rows of `vecs` (cuda fp32 [>= n_rows, dim]) in one launch (crs_mmr_order, csrc/mmr.hip):
    rows int64 / rel fp64 [nq, m_max <= MAX_K], counts int32 [nq], lam = 1 - diversity_penalty -> order int32 [nq, m_max], the
    first counts[i] slots of list i its positions in MMR order, the others -1.  No host sync."""
    import torch
    if out is None:
        out = torch.empty(rows.shape, dtype=torch.int32, device=vecs.device)
    with _translate():
        ops().mmr_order_out(vecs, int(n_rows), rows, rel, counts, float(lam), out)
    return out


def token_match(a, len_a, b, len_b, w_a=None, w_b=None, out=None):
    """BERTScore's greedy matching of n pairs of token states in one launch (crs_token_match, csrc/token_match.hip): a cuda fp32
    [n, seq_a, hidden] (candidates), b [n, seq_b, hidden] (references), len_a / len_b int32 [n], w_a / w_b fp32 [n, seq] token
    weights or None (1 on every real token) -> fp32 [n, 3] = P, R, F.  seq <= 512, hidden a multiple of 64 up to 1024.  No host sync."""
    import torch
    if out is None:
        out = torch.empty((a.shape[0], 3), dtype=torch.float32, device=a.device)
    with _translate():
        ops().token_match_out(a, len_a, b, len_b, w_a, w_b, out)
    return out


def has_rerank_lexical() -> bool:
    """Whether the loaded libcrs_torch.so carries crs::rerank_lexical (a library built before csrc/rerank.hip does not)."""
    return hasattr(ops(), "rerank_lexical")


def rerank_lexical(scores, rows, doc_offsets, doc_tokens, n_rows: int, q_offsets, q_tokens, q_norm, k: int, threshold: float, out=None):
    """Score, threshold and lexically re-rank nq result lists in one launch (crs_rerank_lexical, csrc/rerank.hip): scores fp32 /
    rows int64 [nq, m_max <= MAX_K] (sidecar rows, -1 = empty slot); doc_offsets int64 [>= n_rows + 1] / doc_tokens int32 the rows'
    token CSR; q_offsets int64 [nq + 1] / q_tokens int32 the queries' known token ids; q_norm int32 [nq] -> (order int32 [nq, m_max],
    count int32 [nq], sim fp64 [nq, m_max], rr fp64 [nq, m_max], reranked int32 [nq]), all cuda, in the host rule's bits.  `out`:
    those five tensors, preallocated.  No host sync."""
    import torch
    if out is None:
        nq, dev = rows.shape[0], rows.device
        out = (torch.empty(rows.shape, dtype=torch.int32, device=dev), torch.empty(nq, dtype=torch.int32, device=dev),
               torch.empty(rows.shape, dtype=torch.float64, device=dev), torch.empty(rows.shape, dtype=torch.float64, device=dev),
               torch.empty(nq, dtype=torch.int32, device=dev))
    with _translate():
        ops().rerank_lexical(scores, rows, doc_offsets, doc_tokens, int(n_rows), q_offsets, q_tokens, q_norm, int(k), float(threshold), *out)
    return out


def token_dim_padded(dim: int) -> int:
    """Row length of a token-vector array: dim rounded up to a multiple of 32 (crs_token_project, crs_maxsim)."""
    return (int(dim) + 31) // 32 * 32


def token_project(hidden, w16, bias, dst, out16):
    """Hidden states to packed unit-length fp16 token vectors (crs_token_project, csrc/token_project.hip): hidden cuda fp32
    [n_tok, H], w16 fp16 [dim <= 128, H], bias fp32 [dim] or None, dst int64 [n_tok] (output row of each token, < 0 = drop: that
    hidden row is never read) -> out16 fp16 [rows, token_dim_padded(dim)], written in place: row dst = W h (+ b) scaled to unit
    length, zeros past dim.  The caller keeps every dst below out16's rows (it builds the table on the host).  No host sync."""
    with _translate():
        ops().token_project(hidden, w16, bias, dst, out16)
    return out16


def maxsim(q16, q_len, tok16, n_tokens: int, offsets, n_rows: int, rows, out=None):
    """Late-interaction scores of nq candidate lists in one launch (crs_maxsim, csrc/maxsim.hip): q16 cuda fp16 [nq, lq_max <= 64,
    dimp], q_len int32 [nq], tok16 fp16 [>= n_tokens, dimp] with the CSR offsets int64 [>= n_rows + 1], rows int64 [nq, m_max] ->
    fp32 [nq, m_max]: sum over the query's tokens of the best dot product with a token of the row's document; -inf for a row outside
    [0, n_rows), 0 for an empty document or query.  No host sync."""
    import torch
    if out is None:
        out = torch.empty(rows.shape, dtype=torch.float32, device=rows.device)
    with _translate():
        ops().maxsim(q16, q_len, tok16, int(n_tokens), offsets, int(n_rows), rows, out)
    return out


def pairs_epsilon(row_err: float, pdim: int) -> float:
    """The band that joins the two stages of the near-duplicate join: a pair whose fp32 similarity sim32 is at least
    t has a slab score of at least t - eps, eps = (2 E + E^2)(1 + 1e-4) + (1.5 pdim + 8) 2^-23 with E = row_err the slab's tracked
    row error (|stored row - fp32 row|_2) and pdim its padded row length.  The first term is <c^_i, c^_j> - <c_i, c_j> =
    <c^_i - c_i, c^_j> + <c_i, c^_j - c_j> <= E (1 + E) + E for unit rows (the factor covers norms that are 1 only to fp32
    rounding); the second is the certificate's arithmetic term (csrc/exact.hip exact_err_arith): the fp32 accumulation of the
    slab score and of sim32."""
    e = float(row_err)
    return (2.0 * e + e * e) * (1.0 + 1e-4) + (1.5 * int(pdim) + 8.0) * 2.0 ** -23


def pairs_thresholds(threshold: float, eps: float):
    """(stage 1, stage 2) thresholds as the fp32 values the kernels compare with: the largest fp32 <= threshold - eps, and the
    smallest fp32 >= threshold (sim32 is an fp32: sim32 >= threshold holds exactly when it is at least that value)."""
    import numpy as np
    lo = np.float32(threshold - eps)
    if float(lo) > threshold - eps:
        lo = np.nextafter(lo, np.float32(-np.inf))
    hi = np.float32(threshold)
    if float(hi) < threshold:
        hi = np.nextafter(hi, np.float32(np.inf))
    return float(lo), float(hi)


def pairs_above(slab, n_rows: int, dim: int, a_range, b_range, thr: float, cap: int, out=None):
    """Stage 1 of the near-duplicate join (crs_pairs_above_f16, csrc/join.hip): every pair i < j, i in a_range = (first, rows),
    j in b_range, whose fp16 slab score is >= thr -> (pairs int64 [cap, 2], scores fp32 [cap], count int64 [1]), all cuda; count
    holds the number of qualifying pairs, of which the first min(count, cap) slots are filled in unspecified order (count > cap:
    overflow, re-run with a larger cap).  `out`: the three tensors preallocated, count zeroed.  No host sync."""
    import torch
    if out is None:
        out = (torch.empty((int(cap), 2), dtype=torch.int64, device=slab.device), torch.empty(int(cap), dtype=torch.float32, device=slab.device),
               torch.zeros(1, dtype=torch.int64, device=slab.device))
    with _translate():
        ops().pairs_above_out(slab, int(n_rows), int(dim), int(a_range[0]), int(a_range[1]), int(b_range[0]), int(b_range[1]), float(thr), *out)
    return out


def pairs_verify(pairs, shadow, n_rows: int, thr: float, out=None):
    """Stage 2 (crs_pairs_verify_f32): pairs cuda int64 [m, 2] against the fp32 shadow [>= n_rows, dim] -> (rows_a int64 [m], rows_b
    int64 [m], sims fp32 [m], count int64 [1]): the pairs with sim32 >= thr compacted into the first count slots, in unspecified
    order; sim32 is a fixed-order fp32 dot, bitwise independent of the launch.  `out`: preallocated, count zeroed.  No host sync."""
    import torch
    if out is None:
        m, dev = pairs.shape[0], pairs.device
        out = (torch.empty(m, dtype=torch.int64, device=dev), torch.empty(m, dtype=torch.int64, device=dev),
               torch.empty(m, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
    with _translate():
        ops().pairs_verify_out(pairs, shadow, int(n_rows), float(thr), *out)
    return out


def has_bm25() -> bool:
    """Whether the loaded libcrs_torch.so carries crs::bm25_topk and crs::fuse_rrf (a library built before csrc/bm25.hip does not)."""
    return hasattr(ops(), "bm25_topk") and hasattr(ops(), "fuse_rrf")


def bm25_workspace_bytes(nq: int, k: int, n_rows: int) -> int:
    out = c_size_t(0)
    check(load().crs_bm25_workspace_bytes(int(nq), int(k), int(n_rows), byref(out)))
    return int(out.value)


def bm25_topk(doc_offsets, doc_tokens, doc_tf, doc_len, n_rows: int, q_offsets, q_tokens, q_weights, c0: float, c1: float, k1p1: float,
              k: int, workspace=None, out_scores=None, out_rows=None):
    """Exact BM25 top-k of nq <= 64 queries over the token CSR in one launch chain (crs_bm25_topk, csrc/bm25.hip): doc_offsets int64
    [>= n_rows + 1] / doc_tokens, doc_tf int32 / doc_len int32 [>= n_rows] the rows' tokens, term frequencies and lengths; q_offsets
    int64 [nq + 1] / q_tokens int32 / q_weights fp32 the queries' ascending distinct known ids and their idf weights (at most
    BM25_MAX_PAIRS of them); c0, c1, k1p1 already rounded to fp32 -> (scores fp32 [nq, k], rows int64 [nq, k]), best first, ties by
    lower row, (-inf, -1) past the hits.  All cuda.  No host sync."""
    import torch
    nq, dev = q_offsets.shape[0] - 1, doc_offsets.device
    if workspace is None:
        workspace = torch.empty(bm25_workspace_bytes(nq, k, n_rows), dtype=torch.uint8, device=dev)
    if out_scores is None:
        out_scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
    if out_rows is None:
        out_rows = torch.empty((nq, k), dtype=torch.int64, device=dev)
    with _translate():
        ops().bm25_topk(doc_offsets, doc_tokens, doc_tf, doc_len, int(n_rows), q_offsets, q_tokens, q_weights, float(c0), float(c1),
                        float(k1p1), int(k), workspace, out_scores, out_rows)
    return out_scores, out_rows


def has_sparse() -> bool:
    """Whether the loaded libcrs_torch.so carries the learned-sparse ops (crs::mlm_sparse_pool, crs::sparse_compact, crs::sparse_topk)."""
    return all(hasattr(ops(), n) for n in ("mlm_sparse_pool", "sparse_compact", "sparse_topk"))


def mlm_pool_plan(batch: int, seq: int, hidden: int, vocab: int) -> dict:
    """The launch geometry of crs_mlm_sparse_pool for these sizes (crs_mlm_pool_plan: a pure host call, no device needed)."""
    p = MlmPlan()
    check(load().crs_mlm_pool_plan(int(batch), int(seq), int(hidden), int(vocab), byref(p)))
    return {n: int(getattr(p, n)) for n, _ in MlmPlan._fields_}


def mlm_workspace_bytes(batch: int, seq: int, hidden: int, vocab: int) -> int:
    out = c_size_t(0)
    check(load().crs_mlm_workspace_bytes(int(batch), int(seq), int(hidden), int(vocab), byref(out)))
    return int(out.value)


def mlm_sparse_pool(hidden, lens, transform_w16, transform_bias, ln_gamma, ln_beta, ln_eps: float, decoder_w16, decoder_bias,
                    max_pos: int, workspace=None, out=None):
    """The MLM head of a learned sparse encoder with the max-pool in the projection's epilogue (crs_mlm_sparse_pool,
    csrc/mlm_pool.hip): hidden cuda fp32 [batch, seq, H] final hidden states (padding positions are never read), lens int32 [batch];
    transform_w16 fp16 [H, H], transform_bias / ln_gamma / ln_beta fp32 [H]; decoder_w16 fp16 [V, H], decoder_bias fp32 [V] ->
    out fp32 [batch, Vp >= V] with out[b, v] = log1p(max(0, max_{i < lens[b]} logit[b, i, v])) in columns [0, V); a given `out` keeps
    its other columns.  `workspace` (uint8, mlm_workspace_bytes) afterwards begins with the transform's output as fp16
    [tokens_padded, H].  No host sync."""
    import torch
    batch, seq, H = hidden.shape
    V = decoder_w16.shape[0]
    if workspace is None:
        workspace = torch.empty(mlm_workspace_bytes(batch, seq, H, V), dtype=torch.uint8, device=hidden.device)
    if out is None:
        out = torch.empty((batch, V), dtype=torch.float32, device=hidden.device)
    with _translate():
        ops().mlm_sparse_pool(hidden, lens, transform_w16, transform_bias, ln_gamma, ln_beta, float(ln_eps), decoder_w16, decoder_bias,
                              int(max_pos), workspace, out)
    return out


def sparse_compact(weights, vocab: int, cap: int, skip_ids=None, out=None):
    """Dense non-negative weight rows to bounded sparse rows (crs_sparse_compact, csrc/sparse_compact.hip): weights cuda fp32
    [batch, Vp >= vocab]; per row the ids with weight > 0 that are not in skip_ids (int32, at most SPARSE_MAX_SKIP), the `cap` largest
    when there are more (ties by lower id), in ascending id order -> (ids int32 [batch, cap], weights fp32 [batch, cap], counts int32
    [batch]); unused slots are (-1, 0).  Exact.  No host sync."""
    import torch
    batch, dev = weights.shape[0], weights.device
    if out is None:
        out = (torch.empty((batch, cap), dtype=torch.int32, device=dev), torch.empty((batch, cap), dtype=torch.float32, device=dev),
               torch.empty(batch, dtype=torch.int32, device=dev))
    with _translate():
        ops().sparse_compact(weights, int(vocab), skip_ids, *out)
    return out


def sparse_workspace_bytes(nq: int, k: int, n_rows: int) -> int:
    out = c_size_t(0)
    check(load().crs_sparse_workspace_bytes(int(nq), int(k), int(n_rows), byref(out)))
    return int(out.value)


def sparse_topk(doc_offsets, doc_tokens, doc_weights, n_rows: int, q_offsets, q_tokens, q_weights, k: int, workspace=None,
                out_scores=None, out_rows=None):
    """Exact impact (sparse dot product) top-k of nq <= 64 queries over a weighted token CSR in one launch chain (crs_sparse_topk,
    csrc/sparse_scan.hip): doc_offsets int64 [>= n_rows + 1] / doc_tokens int32 / doc_weights fp32 the rows' ascending ids and their
    weights; q_offsets int64 [nq + 1] / q_tokens int32 / q_weights fp32 the queries' (at most BM25_MAX_PAIRS entries) -> (scores fp32
    [nq, k], rows int64 [nq, k]), best first, ties by lower row, (-inf, -1) past the hits.  All cuda.  No host sync."""
    import torch
    nq, dev = q_offsets.shape[0] - 1, doc_offsets.device
    if workspace is None:
        workspace = torch.empty(sparse_workspace_bytes(nq, k, n_rows), dtype=torch.uint8, device=dev)
    if out_scores is None:
        out_scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
    if out_rows is None:
        out_rows = torch.empty((nq, k), dtype=torch.int64, device=dev)
    with _translate():
        ops().sparse_topk(doc_offsets, doc_tokens, doc_weights, int(n_rows), q_offsets, q_tokens, q_weights, int(k), workspace, out_scores,
                          out_rows)
    return out_scores, out_rows


def fuse_rrf(dense_rows, lex_rows, k_out: int, c: float = 60.0, w_dense: float = 1.0, w_lex: float = 1.0, out=None):
    """Weighted reciprocal rank fusion of nq (dense, lexical) list pairs in one launch (crs_fuse_rrf, csrc/fuse.hip): dense_rows int64
    [nq, m_dense <= MAX_K], lex_rows int64 [nq, m_lex <= MAX_K] (rank order, -1 = empty slot) -> (rows int64, fused fp64, dense_pos
    int32, lex_pos int32, each [nq, k_out]; count int32 [nq]), all cuda, in the host rule's bits.  `out`: those five tensors,
    preallocated.  No host sync."""
    import torch
    if out is None:
        nq, dev = dense_rows.shape[0], dense_rows.device
        out = (torch.empty((nq, k_out), dtype=torch.int64, device=dev), torch.empty((nq, k_out), dtype=torch.float64, device=dev),
               torch.empty((nq, k_out), dtype=torch.int32, device=dev), torch.empty((nq, k_out), dtype=torch.int32, device=dev),
               torch.empty(nq, dtype=torch.int32, device=dev))
    with _translate():
        ops().fuse_rrf(dense_rows, lex_rows, float(c), float(w_dense), float(w_lex), *out)
    return out


def wordpiece_encode(text, offsets, n_bytes: int, table, rep_pool, slots, vocab_pool, max_probe: int, lmax: int, mode: int, unk_id: int,
                     cls_id: int, sep_id: int, pad_id: int, hash_lo: int, hash_span: int, max_len: int, out=None):
    """Tokenise n UTF-8 texts in one launch (crs_wordpiece_encode, csrc/wordpiece.hip): text uint8 [>= n_bytes] the texts' bytes end to
    end, offsets int64 [n + 1]; table / rep_pool / slots / vocab_pool the int32 tensors of rag/_wordpiece.py; mode 0 WordPiece, 1 the
    HashTokenizer rule -> (ids int32 [n, max_len]: cls, ids, sep, pad; lens int32 [n]; flags int32 [n]: 1 = tokenise this text on the
    host instead).  All cuda.  `out`: those three, preallocated.  No host sync; a missing kernel raises."""
    import torch
    n, dev = offsets.shape[0] - 1, text.device
    if out is None:
        out = (torch.empty((n, int(max_len)), dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
               torch.empty(n, dtype=torch.int32, device=dev))
    with _translate():
        ops().wordpiece_encode(text, offsets, int(n_bytes), table, rep_pool, slots, vocab_pool, int(max_probe), int(lmax), int(mode),
                               int(unk_id), int(cls_id), int(sep_id), int(pad_id), int(hash_lo), int(hash_span), *out)
    return out


def unigram_encode(text, offsets, n_bytes: int, table, rep_pool, slots, slot_scores, vocab_pool, max_probe: int, lmax: int,
                   unk_score: float, opts: int, unk_id: int, cls_id: int, sep_id: int, pad_id: int, max_len: int, out=None):
    """Tokenise n UTF-8 texts in one launch (crs_unigram_encode, csrc/unigram.hip): text / offsets as wordpiece_encode; table /
    rep_pool / slots / vocab_pool int32 and slot_scores fp64, the tensors of rag/_unigram.py; opts the UNIGRAM_* bits -> (ids int32
    [n, max_len]: <s>, ids, </s>, pad; lens int32 [n]; flags int32 [n]: 1 = tokenise this text on the host instead).  All cuda.
    No host sync; a missing kernel raises."""
    import torch
    n, dev = offsets.shape[0] - 1, text.device
    if out is None:
        out = (torch.empty((n, int(max_len)), dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
               torch.empty(n, dtype=torch.int32, device=dev))
    with _translate():
        ops().unigram_encode(text, offsets, int(n_bytes), table, rep_pool, slots, slot_scores, vocab_pool, int(max_probe), int(lmax),
                             float(unk_score), int(opts), int(unk_id), int(cls_id), int(sep_id), int(pad_id), *out)
    return out


def rescore_f32(q32, shadow, n_rows: int, id_base: int, scores, ids) -> None:
    """In-place variant kept from ABI v1 (C ABI only): re-score all k candidates and re-sort each row."""
    nq, dim = q32.shape
    k = scores.shape[1]
    check(load().crs_rescore_f32(_ptr(q32), nq, dim, _ptr(shadow), n_rows, id_base, k, _ptr(scores),
                                 _ptr(ids), _stream_ptr()))


def score_rows_f32(q32, shadow, n_rows: int, id_base: int, ids):
    """fp32 scores of candidate lists of any length: ids int64 [nq, k] -> fp32 [nq, k] (-inf where ids < 0)."""
    import torch
    scores = torch.full(ids.shape, float("-inf"), dtype=torch.float32, device=q32.device)
    with _translate():
        ops().score_rows_f32_out(q32, shadow, int(n_rows), int(id_base), ids.contiguous(), scores)
    return scores


def refine_f32(q32, shadow, n_rows: int, id_base: int, cand_ids, k_out: int, out_scores=None, out_ids=None):
    """Exact fp32 re-rank of over-fetched candidates: cand_ids int64 [nq, k_in] (what cosine_topk found in the
    fp16/int8 slab) -> the k_out best by <q32, shadow[id - id_base]> (score desc, id asc)."""
    import torch
    nq, dim = q32.shape
    if out_scores is None:
        out_scores = torch.empty((nq, k_out), dtype=torch.float32, device=q32.device)
    if out_ids is None:
        out_ids = torch.empty((nq, k_out), dtype=torch.int64, device=q32.device)
    with _translate():
        ops().refine_f32_out(q32, shadow, int(n_rows), int(id_base), cand_ids, int(k_out), out_scores, out_ids)
    return out_scores, out_ids


def overfetch(nq: int, top_k: int, want: int = 24, n_rows: int = 1 << 62, slab_type: int = SLAB_F16) -> int:
    """Candidates the scan fetches for the fp32 re-rank (never below top_k, never above MAX_K).
    `want` (24) on shards of >= 4 M rows, where the top scores crowd together (10 M x 384: about 1e-3 apart at rank 10; the gap
    from rank 10 to rank 24 is ~9e-3 against a certificate bound of ~6e-4): all 8192 benchmark queries certify with 24 as with 32
    candidates, while with 16 about 3e-4 of them would escalate -- a second sweep of the whole shard each.  Same box, C4 batch:
    1.408 / 1.432 / 1.451 ms at 16 / 24 / 32 (chain slots, tile refine and merge grow with the length).  16 on smaller shards: the
    same gaps are wider (fewer rows in the tail), an escalation sweep is short, and 32 candidates measured 16 % of a 1.25 M-row
    shard's batch (0.301 -> 0.259 ms: one rank of an 8-GPU step).  Launches of more than 64 queries keep to 16 when top_k
    allows: the large-batch kernels (scan_wide.hip) carry a 16-slot chain, and 32 candidates would send those launches to the
    64-query kernel once per query block.  int8 slabs: 16 -- their certificate is too wide to hold at either length
    (0.07 % / 34 % of C5's queries at 16 / 32), the empirical Recall@10 is 1.0 on 8192 queries at both, and the 32-slot chain makes the
    issue-bound int8 kernel 6 % slower (C5 31.3 -> 33.5 k q/s).
    Above top_k 10 the margin grows with top_k: k' >= ceil(1.6 top_k) (capped at MAX_K).  k' == top_k would leave the re-rank
    nothing to re-rank and the certificate nothing to stand on: every query escalated on fp16, the slab's own order on int8.
    1.6 is the ratio top_k 10 already runs at (16 / 10), so the lengths up to top_k 10 stay as above.  Measured on 1 M x 384
    fp16 rows, 64 queries (half planted near a row): every query certified at k' = 1.4, 1.6, 2 and 2.4 x top_k for each
    top_k from 10 to 40."""
    want = int(want)
    if n_rows < 4_000_000 or (nq > 64 and top_k <= 16) or slab_type == SLAB_I8:
        want = min(want, 16)
    return min(MAX_K, max(int(top_k), want, -(-8 * int(top_k) // 5)))


def exact_workspace_bytes(nq: int, cap: int = EXACT_CAP) -> int:
    return int(load().crs_exact_workspace_bytes(int(nq), int(cap)))


def exact_row_error_bound(dim: int, slab_type: int) -> float:
    """Analytic worst case of |stored row - fp32 row|_2 (used when a slab did not track it)."""
    return float(load().crs_exact_row_error_bound(int(dim), int(slab_type)))


def refine_f32_cert(q32, q16, shadow, n_rows: int, id_base: int, cand_ids, cand_scores, k_out: int, row_err_max: float,
                    slab_type: int, exact_ws, cap: int = EXACT_CAP, out_scores=None, out_ids=None, status=None):
    """crs_refine_f32 + the per-query exactness proof: returns (scores [nq, k_out], ids [nq, k_out], status int32 [nq])
    with status 0 = the list is provably the fp32 top-k of all n_rows rows, 1 = not proven (feed escalate_exact)."""
    import torch
    nq = q32.shape[0]
    if out_scores is None:
        out_scores = torch.empty((nq, k_out), dtype=torch.float32, device=q32.device)
    if out_ids is None:
        out_ids = torch.empty((nq, k_out), dtype=torch.int64, device=q32.device)
    if status is None:
        status = torch.empty(nq, dtype=torch.int32, device=q32.device)
    with _translate():
        ops().refine_f32_cert_out(q32, q16, shadow, int(n_rows), int(id_base), cand_ids, cand_scores, int(k_out),
                                  float(row_err_max), int(slab_type), out_scores, out_ids, status, exact_ws, int(cap))
    return out_scores, out_ids, status


def cosine_topk_cert(q32, q16, slab, shadow, n_rows: int, dim: int, k_in: int, k_out: int, row_err_max: float, exact_ws,
                     cap: int = EXACT_CAP, *, scales=None, id_base: int = 0, workspace=None, cand_scores=None, cand_ids=None,
                     out_scores=None, out_ids=None, status=None):
    """cosine_topk with k = k_in followed by refine_f32_cert, in one call (crs_cosine_topk_cert: one fused tail kernel after the
    scan where the plan allows).  q32: the unit fp32 queries [nq, dim]; q16: the scan's query block.  Returns (scores [nq, k_out],
    ids [nq, k_out], status int32 [nq]); cand_scores / cand_ids [nq, k_in] receive the k_in candidates of the slab."""
    import torch
    nq = q32.shape[0]
    dev = q32.device
    need = scan_workspace_bytes(nq, dim, k_in, n_rows)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    if cand_scores is None:
        cand_scores = torch.empty((nq, k_in), dtype=torch.float32, device=dev)
    if cand_ids is None:
        cand_ids = torch.empty((nq, k_in), dtype=torch.int64, device=dev)
    if out_scores is None:
        out_scores = torch.empty((nq, k_out), dtype=torch.float32, device=dev)
    if out_ids is None:
        out_ids = torch.empty((nq, k_out), dtype=torch.int64, device=dev)
    if status is None:
        status = torch.empty(nq, dtype=torch.int32, device=dev)
    with _translate():
        ops().cosine_topk_cert_out(q32, q16, slab, scales, shadow, int(n_rows), int(id_base), int(k_out), float(row_err_max), workspace,
                                   cand_scores, cand_ids, out_scores, out_ids, status, exact_ws, int(cap))
    return out_scores, out_ids, status


def escalate_exact(q32, q16, slab, shadow, n_rows: int, id_base: int, k_out: int, out_scores, out_ids, status, exact_ws,
                   cap: int = EXACT_CAP, scales=None) -> None:
    """Make every status-1 query of a refine_f32_cert result exact, in place, on the current stream (no host sync;
    returns at once on the device when nothing is to do).  status 2 afterwards = list longer than cap."""
    with _translate():
        ops().escalate_exact(q32, q16, slab, scales, shadow, int(n_rows), int(id_base), int(k_out), out_scores, out_ids,
                             status, exact_ws, int(cap))


def large_k_plan(k_out: int, n_rows: int):
    """The partition of crs_cosine_topk_large_cert (crs_large_k_plan): (parts, chunk_rows).  P = clamp(ceil(k_out / 16), 2, 64)
    chunks are asked for; chunk_rows = ceil(n_rows / P) rounded up to a multiple of 16, so a small shard gets fewer chunks.  Chunk
    p holds rows [p chunk_rows, min(n_rows, (p + 1) chunk_rows)); each is scanned for its 64 best, so parts x 64 <= 4096
    candidates per query, each chunk's list about 4 x its expected share of the top-k_out."""
    k_out, n_rows = int(k_out), int(n_rows)
    p = min(LARGE_K_MAX_PARTS, max(2, -(-k_out // 16)))
    rows = -(-(-(-n_rows // p)) // 16) * 16
    return -(-n_rows // rows), rows


def large_k_cand_bytes(nq: int, k_out: int, n_rows: int) -> int:
    """Bytes of the [parts, nq, 64] candidate block at the head of the large-k workspace: scores fp32 | ids int64, each 256-aligned."""
    parts, _ = large_k_plan(k_out, n_rows)
    slots = parts * int(nq) * MAX_K
    return -(-slots * 4 // 256) * 256 + -(-slots * 8 // 256) * 256


def large_cert_workspace_bytes(nq: int, dim: int, k_out: int, n_rows: int) -> int:
    """crs_cosine_topk_large_cert_workspace_bytes: the candidate block + one workspace the chunk scans share."""
    out = c_size_t(0)
    check(load().crs_cosine_topk_large_cert_workspace_bytes(int(nq), int(dim), int(k_out), int(n_rows), byref(out)))
    return int(out.value)


def cosine_topk_large_cert(q32, q16, slab, shadow, n_rows: int, dim: int, k_out: int, row_err_max: float, exact_ws,
                           cap: int = EXACT_CAP, *, scales=None, id_base: int = 0, workspace=None, out_scores=None, out_ids=None,
                           status=None):
    """Certified fp32 top-k_out for k_out up to MAX_K_CERT: the partitioned over-fetch (large_k_plan) of the slab, its fp32 re-rank
    and the per-query proof (crs_cosine_topk_large_cert).  Returns (scores [nq, k_out], ids [nq, k_out], status int32 [nq]) like
    cosine_topk_cert; escalate_exact (same k_out, cap >= k_out) makes status-1 queries exact."""
    import torch
    nq = q32.shape[0]
    dev = q32.device
    need = large_cert_workspace_bytes(nq, dim, k_out, n_rows)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    if out_scores is None:
        out_scores = torch.empty((nq, k_out), dtype=torch.float32, device=dev)
    if out_ids is None:
        out_ids = torch.empty((nq, k_out), dtype=torch.int64, device=dev)
    if status is None:
        status = torch.empty(nq, dtype=torch.int32, device=dev)
    with _translate():
        ops().cosine_topk_large_cert_out(q32, q16, slab, scales, shadow, int(n_rows), int(id_base), int(k_out), float(row_err_max),
                                         workspace, out_scores, out_ids, status, exact_ws, int(cap))
    return out_scores, out_ids, status


def refine_large_cert(q32, q16, shadow, n_rows: int, id_base: int, cand_ids, cand_scores, chunk_rows: int, k_out: int,
                      row_err_max: float, slab_type: int, exact_ws, cap: int = EXACT_CAP):
    """The re-rank + certificate kernel of cosine_topk_large_cert alone, on a candidate block the caller holds: cand_ids /
    cand_scores [parts, nq, 64], block p = the slab top-64 of rows [p chunk_rows, (p + 1) chunk_rows) + id_base."""
    import torch
    nq = q32.shape[0]
    out_scores = torch.empty((nq, k_out), dtype=torch.float32, device=q32.device)
    out_ids = torch.empty((nq, k_out), dtype=torch.int64, device=q32.device)
    status = torch.empty(nq, dtype=torch.int32, device=q32.device)
    with _translate():
        ops().refine_large_cert_out(q32, q16, shadow, int(n_rows), int(id_base), cand_ids.contiguous(), cand_scores.contiguous(),
                                    int(chunk_rows), int(k_out), float(row_err_max), int(slab_type), out_scores, out_ids, status,
                                    exact_ws, int(cap))
    return out_scores, out_ids, status


class WireBlock:
    """One rank's per-shard result in the one-collective wire layout of include/crs_hip.h:
    [ids int64 [nq, k] | scores fp32 [nq, k] | pad].  `.ids` / `.scores` are views into `.buf`, so the
    search kernels write the block in place and `buf` is what the all-gather sends."""

    def __init__(self, nq: int, k: int, device, world: int = 1, gather: bool = False):
        import torch
        lib = load()
        self.nq, self.k, self.world = nq, k, world
        self.nbytes = int(lib.crs_wire_bytes(nq, k))
        off = int(lib.crs_wire_scores_offset(nq, k))
        self.buf = torch.zeros(self.nbytes, dtype=torch.uint8, device=device)
        self.ids = self.buf[:off].view(torch.int64).view(nq, k)
        self.scores = self.buf[off:off + nq * k * 4].view(torch.float32).view(nq, k)
        self.gathered = torch.zeros(world * self.nbytes, dtype=torch.uint8, device=device) if (world > 1 or gather) else None


def merge_topk_wire(gathered, nlists: int, nq: int, k_in: int, k_out: int, out_scores=None, out_ids=None):
    """gathered: cuda uint8 [nlists * crs_wire_bytes(nq, k_in)] (the all-gathered WireBlocks) -> global top-k_out."""
    import torch
    out_s = out_scores if out_scores is not None else torch.empty((nq, k_out), dtype=torch.float32, device=gathered.device)
    out_i = out_ids if out_ids is not None else torch.empty((nq, k_out), dtype=torch.int64, device=gathered.device)
    with _translate():
        ops().merge_topk_wire_out(gathered, int(nlists), int(nq), int(k_in), int(k_out), out_s, out_i)
    return out_s, out_i


def merge_sorted_wire(gathered, nlists: int, nq: int, k_in: int, k_out: int, out_scores=None, out_ids=None):
    """merge_sorted over the all-gathered WireBlocks (cuda uint8 [nlists * crs_wire_bytes(nq, k_in)])."""
    import torch
    out_s = out_scores if out_scores is not None else torch.empty((nq, k_out), dtype=torch.float32, device=gathered.device)
    out_i = out_ids if out_ids is not None else torch.empty((nq, k_out), dtype=torch.int64, device=gathered.device)
    with _translate():
        ops().merge_sorted_wire_out(gathered, int(nlists), int(nq), int(k_in), int(k_out), out_s, out_i)
    return out_s, out_i


def cu_masked_stream(first_cu: int, n_cus: int, device=None):
    """A torch stream whose kernels run on CUs [first_cu, first_cu + n_cus) only (crs_stream_create_cu_masked).  The HIP stream
    lives as long as the process (a handful per engine)."""
    import torch
    out = c_void_p(0)
    check(load().crs_stream_create_cu_masked(int(first_cu), int(n_cus), byref(out)))
    return torch.cuda.ExternalStream(int(out.value), device=device)


def scan_plan_describe(nq: int, dim: int, k: int, n_rows: int, slab_type: int = SLAB_F16) -> str:
    """Kernel family + launch geometry crs_cosine_topk would use (for bench lines and profiles)."""
    buf = ctypes.create_string_buffer(256)
    check(load().crs_scan_plan_describe(nq, dim, k, n_rows, slab_type, buf, 256))
    return buf.value.decode()


def encoder_plan_describe(desc, batch: int, seq: int, rel_bias: bool = False, pair: int = 0) -> str:
    """One line per launch of embedding, one layer and the tail of a forward, in launch order (crs_encoder_plan_describe): kernel with
    its template arguments, grid in workgroups, workgroup size, dynamic LDS bytes.  desc: the ctypes crs_encoder_desc (HipEncoder.desc);
    pair: 0 pooling tail, 1 pair head with type ids, 2 pair head without."""
    cap = 2048
    while True:
        buf = ctypes.create_string_buffer(cap)
        need = load().crs_encoder_plan_describe(byref(desc), int(batch), int(seq), int(bool(rel_bias)), int(pair), buf, cap)
        check(min(need, 0))
        if need < cap:
            return buf.value.decode()
        cap = need + 1


def time_cosine_topk(q16, slab, n_rows: int, dim: int, k: int, iters: int, *, slab_type: int = SLAB_F16,
                     scales=None):
    """hipEvent-timed launches on the current stream: returns (ms per scan+merge, ms per scan kernel)."""
    import torch
    nq = q16.shape[0]
    need = scan_workspace_bytes(nq, dim, k, n_rows)
    ws = torch.empty(need, dtype=torch.uint8, device=q16.device)
    out_s = torch.empty((nq, k), dtype=torch.float32, device=q16.device)
    out_i = torch.empty((nq, k), dtype=torch.int64, device=q16.device)
    ms_total, ms_scan = c_float(0), c_float(0)
    check(load().crs_time_cosine_topk(_ptr(q16), nq, dim, slab_type, _ptr(slab), _ptr(scales), n_rows, k,
                                      _ptr(ws), ws.numel(), _ptr(out_s), _ptr(out_i), _stream_ptr(),
                                      iters, byref(ms_total), byref(ms_scan)))
    return float(ms_total.value), float(ms_scan.value)
