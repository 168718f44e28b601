"""CPU: the fp8 late-interaction sweep's plan as a pure function, the reranker's token_dtype option, and the new symbols."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_Q = 8      # kMsF8GroupQ


def _plan(nq, row_count, dimp=128, k=10):
    from rag import _native as nat
    line = nat.maxsim_topk_plan_describe(nq, 32, dimp, k, row_count, f8=True)
    m = re.search(r"maxsim_scan_f8<dimp=(\d+)> grid=(\d+)x(\d+) .*queries/wave=(\d+) .*kp=(\d+) lds=(\d+)", line)
    return tuple(int(x) for x in m.groups())


@pytest.mark.parametrize("nq, qgroups", [(1, 1), (GROUP_Q, 1), (GROUP_Q + 1, 2), (64, 8)])
def test_grid_at_the_group_boundary(nq, qgroups):
    dimp, g, gy, per_wave, kp, lds = _plan(nq, 100000)
    assert (dimp, gy, per_wave * 4, kp) == (128, qgroups, GROUP_Q, 32)
    assert lds == 2 * 256 * 128                               # two windows of 256 rows of dimp BYTES: half the fp16 sweep's
    assert g == -(-512 // qgroups)
    assert _plan(nq, 65)[1] == 2 and _plan(nq, 100000, dimp=32, k=33)[4:] == (64, 2 * 256 * 32)


def test_workspace_bound_is_monotone_and_covers_the_plan():
    from rag import _native as nat
    last = 0
    for nq, k, rows in [(1, 1, 1), (1, 1, 64), (1, 32, 65), (8, 32, 65), (9, 33, 65), (9, 64, 10 ** 6), (300, 64, 10 ** 6), (300, 64, 2 ** 32 - 1)]:
        b = nat.maxsim_topk_workspace_bytes(nq, k, rows, f8=True)
        assert b >= last
        last = b
        _, g, _, _, kp, _ = _plan(nq, rows, k=k)
        assert b >= g * nq * kp * 12
    with pytest.raises(nat.NativeError, match="row_count"):
        nat.maxsim_topk_workspace_bytes(1, 1, 2 ** 32, f8=True)


def test_token_dtype_is_validated():
    from rag.late_interaction import LateInteractionReranker
    cfg = {"model_name": "synthetic:tiny-colbert"}
    assert LateInteractionReranker(cfg).token_dtype == "fp16"
    assert LateInteractionReranker({**cfg, "token_dtype": "fp8"}).token_dtype == "fp8"
    for bad in ("int8", "FP8", None, 8):
        with pytest.raises(ValueError, match="token_dtype"):
            LateInteractionReranker({**cfg, "token_dtype": bad})


def test_new_symbols_are_declared_exported_and_bound():
    import torch
    from rag import _native as nat
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crs_hip.h")).read(), flags=re.S)
    lib = nat.load()
    for name in ("crs_token_project_f8", "crs_maxsim_f8", "crs_maxsim_topk_f8", "crs_maxsim_topk_f8_workspace_bytes",
                 "crs_maxsim_topk_f8_plan_describe"):
        assert re.search(r"\bint %s\s*\(" % name, header) and hasattr(lib, name) and name in nat.exported_symbols(), name
    assert lib.crs_abi_version() == 3
    nat.ops()
    assert str(torch.ops.crs.maxsim_f8.default._schema) == \
        "crs::maxsim_f8(Tensor q8, Tensor q_len, Tensor tok8, int n_tokens, Tensor offsets, int n_rows, Tensor rows, Tensor(a!) out) -> ()"
    assert hasattr(torch.ops.crs, "token_project_f8") and hasattr(torch.ops.crs, "maxsim_topk_f8")
