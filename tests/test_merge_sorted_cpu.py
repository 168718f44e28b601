"""CPU: the sorted-list merge entry points (crs_merge_sorted, crs_merge_sorted_wire) are declared, exported and bound, the ABI
version did not move, and their argument checks answer CRS_EINVAL before any HIP call."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("crs_merge_sorted", "crs_merge_sorted_wire")


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
    # same argument order as the k <= 64 neighbours
    assert nat._SIGNATURES["crs_merge_sorted"] == nat._SIGNATURES["crs_merge_topk"]
    assert nat._SIGNATURES["crs_merge_sorted_wire"] == nat._SIGNATURES["crs_merge_topk_wire"]
    ops = nat.ops()
    for name in ("merge_sorted_out", "merge_sorted_wire_out"):
        assert hasattr(ops, name), name
    assert "Tensor scores, Tensor ids, int k_out" in str(torch.ops.crs.merge_sorted_out.default._schema)
    assert callable(nat.merge_sorted) and callable(nat.merge_sorted_wire)
    assert nat.MAX_K == 64 and nat.MAX_K_CERT == 1024 and nat.MERGE_SORTED_MAX_LISTS == 64


def test_argument_validation_without_gpu():
    from rag import _native as nat
    lib = nat.load()
    buf = (ctypes.c_char * 4096)()                     # host memory standing in for device pointers: never dereferenced
    p = ctypes.cast(buf, ctypes.c_void_p)
    EINVAL = -1
    # crs_merge_sorted(scores, ids, nlists, nq, k_in, k_out, out_scores, out_ids, stream)
    for nlists, nq, k_in, k_out in ((0, 1, 8, 8), (65, 1, 8, 8), (-1, 1, 8, 8), (2, 0, 8, 8), (2, 1, 0, 8), (2, 1, 1025, 8), (2, 1, 8, 0),
                                    (2, 1, 8, 1025), (2, 1 << 30, 8, 8)):
        assert lib.crs_merge_sorted(p, p, nlists, nq, k_in, k_out, p, p, None) == EINVAL, (nlists, nq, k_in, k_out)
        assert b"bad sizes" in lib.crs_last_error() and b"CRS_MAX_K_CERT" in lib.crs_last_error()
        assert lib.crs_merge_sorted_wire(p, nlists, nq, k_in, k_out, p, p, None) == EINVAL, (nlists, nq, k_in, k_out)
        assert b"bad sizes" in lib.crs_last_error()
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert lib.crs_merge_sorted(args[0], args[1], 2, 1, 100, 100, args[2], args[3], None) == EINVAL
        assert b"null pointer" in lib.crs_last_error()
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.crs_merge_sorted_wire(args[0], 2, 1, 100, 100, args[1], args[2], None) == EINVAL
        assert b"null pointer" in lib.crs_last_error()
    odd = ctypes.c_void_p((p.value + 15) // 16 * 16 + 4)
    assert lib.crs_merge_sorted_wire(odd, 2, 1, 100, 100, p, p, None) == EINVAL
    assert b"8-byte aligned" in lib.crs_last_error()
    # the k <= 64 entry points keep their limit and their words
    assert lib.crs_merge_topk(p, p, 2, 1, 100, 100, p, p, None) == EINVAL
    assert lib.crs_last_error() == b"bad sizes (k_out <= CRS_MAX_K)"
    assert lib.crs_merge_topk_wire(p, 2, 1, 100, 100, p, p, None) == EINVAL
    assert lib.crs_last_error() == b"bad sizes (k_out <= CRS_MAX_K)"
