"""CPU: the late-interaction sweep without a device -- its three entry points are declared, exported and bound; every argument
check of crs_maxsim_topk answers CRS_EINVAL with its message before any HIP call; the workspace grows with nq, k and row_count; the
plan line needs no device."""
import ctypes
import os

import pytest

NAMES = ("crs_maxsim_topk_workspace_bytes", "crs_maxsim_topk_plan_describe", "crs_maxsim_topk")


def test_declared_exported_and_bound():
    import torch
    from rag import _native as nat
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "crs_hip.h")).read()
    lib = nat.load()
    for name in NAMES:
        assert name + "(" in header and name in nat.exported_symbols() and hasattr(lib, name)
    assert "#define CRS_MAXSIM_SCAN_WINDOW 256" in header and "#define CRS_MAXSIM_SCAN_ITEM_ROWS 64" in header
    assert nat.MAXSIM_SCAN_WINDOW == 256 and nat.MAXSIM_SCAN_ITEM_ROWS == 64 and callable(nat.maxsim_topk)
    nat.ops()
    assert "row_first" in str(torch.ops.crs.maxsim_topk.default._schema)


def test_argument_checks_answer_einval_before_any_hip_call():
    from rag import _native as nat
    lib = nat.load()
    buf = (ctypes.c_char * 4096)()                     # host memory standing in for device pointers: never dereferenced
    p = ctypes.c_void_p((ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 2)
    names = ("q16", "q_len", "nq", "lq_max", "tok16", "offsets", "n_rows", "n_tokens", "row_first", "row_count", "dimp", "k", "ws",
             "ws_bytes", "out_s", "out_r")
    good = dict(q16=p, q_len=p, nq=0, lq_max=32, tok16=p, offsets=p, n_rows=1000, n_tokens=5000, row_first=0, row_count=1000, dimp=128,
                k=10, ws=p, ws_bytes=1 << 30, out_s=p, out_r=p)

    def topk(**change):
        args = dict(good, **change)
        return lib.crs_maxsim_topk(*[args[n] for n in names], None)

    for bad, word in (({"lq_max": 0}, b"lq_max"), ({"lq_max": 65}, b"lq_max"), ({"dimp": 48}, b"dimp"), ({"dimp": 160}, b"dimp"),
                      ({"k": 0}, b"k must"), ({"k": 65}, b"k must"), ({"nq": -1}, b"nq"), ({"nq": 65536}, b"nq"),
                      ({"row_first": -1}, b"row range"), ({"row_count": -1}, b"row range"), ({"row_first": 1}, b"row range"),
                      ({"row_first": 1001, "row_count": 0}, b"row range"), ({"q16": None}, b"q16_dev"), ({"q_len": None}, b"q_len_dev"),
                      ({"offsets": None}, b"offsets_dev"), ({"tok16": None}, b"tok16_dev"), ({"ws": None}, b"workspace_dev"),
                      ({"out_s": None}, b"out_scores_dev"), ({"out_r": None}, b"out_scores_dev"), ({"q16": odd}, b"aligned"),
                      ({"tok16": odd}, b"aligned"), ({"ws": odd}, b"aligned"), ({"nq": 9, "ws_bytes": 1024}, b"workspace too small")):
        assert topk(**bad) == -1, bad
        assert word in lib.crs_last_error(), (bad, lib.crs_last_error())
    assert topk() == 0                                                   # nq 0: nothing to do, no launch
    assert topk(tok16=None, n_tokens=0) == 0                             # an empty token array may be null


def test_workspace_grows_with_every_argument_and_the_plan_needs_no_device():
    from rag import _native as nat
    ws = nat.maxsim_topk_workspace_bytes
    for lo, hi in zip((1, 7, 8, 9, 64, 511, 4096), (7, 8, 9, 64, 511, 4096, 65535)):
        for rows in (0, 1, 64, 65, 10_000, 10_000_000):
            assert ws(lo, 10, rows) <= ws(hi, 10, rows), (lo, hi, rows)
    for rows_lo, rows_hi in zip((0, 1, 64, 65, 10_000), (1, 64, 65, 10_000, 10_000_000)):
        for nq in (1, 9, 1000):
            assert ws(nq, 10, rows_lo) <= ws(nq, 10, rows_hi)
            assert ws(nq, 1, rows_hi) <= ws(nq, 32, rows_hi) <= ws(nq, 33, rows_hi) <= ws(nq, 64, rows_hi)
    assert ws(9, 64, 10_000_000) > ws(9, 10, 64) > 0
    with pytest.raises(Exception, match="k must"):
        ws(1, 65, 10)
    line = nat.maxsim_topk_plan_describe(9, 32, 128, 10, 1_000_000)
    assert "maxsim_scan<ksteps=4>" in line and "grid=256x2" in line and "kp=32" in line and "lds=131072" in line
    assert "grid=3x1" in nat.maxsim_topk_plan_describe(1, 64, 32, 64, 150) and "kp=64" in nat.maxsim_topk_plan_describe(1, 64, 32, 33, 150)
