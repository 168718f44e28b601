"""CPU: the res2 late-interaction sweep's plan as a pure function, the reranker's token_dtype 'res2' and codec keys, the codec's
centroid count, and the new symbols."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_Q = 8      # kMsRcGroupQ


def _plan(nq, row_count, dimp=128, k=10):
    from rag import _native as nat
    line = nat.maxsim_topk_rc_plan_describe(nq, 32, dimp, k, row_count)
    m = re.search(r"maxsim_scan_rc<dimp=(\d+)> grid=(\d+)x(\d+) .*queries/wave=(\d+) .*kp=(\d+) lds=(\d+)", line)
    return tuple(int(x) for x in m.groups())


@pytest.mark.parametrize("nq, qgroups", [(1, 1), (GROUP_Q, 1), (GROUP_Q + 1, 2), (64, 8)])
def test_grid_at_the_group_boundary(nq, qgroups):
    dimp, g, gy, per_wave, kp, lds = _plan(nq, 100000)
    assert (dimp, gy, per_wave * 4, kp) == (128, qgroups, GROUP_Q, 32)
    assert lds == 2 * 256 * (128 // 4 + 6)                    # two windows of 256 code rows, cids and scales: no centroid rows
    assert g == -(-512 // qgroups)
    assert _plan(nq, 65)[1] == 2 and _plan(nq, 100000, dimp=32, k=33)[4:] == (64, 2 * 256 * 14)
    from rag import _native as nat
    assert nat.maxsim_topk_rc_workspace_bytes(nq, 10, 100000) >= g * nq * kp * 12
    with pytest.raises(nat.NativeError, match="row_count"):
        nat.maxsim_topk_rc_workspace_bytes(1, 1, 2 ** 32)


def test_token_dtype_res2_and_the_codec_keys_are_validated():
    from rag import _token_codec as tc
    from rag.late_interaction import LateInteractionReranker
    cfg = {"model_name": "synthetic:tiny-colbert", "token_dtype": "res2"}
    li = LateInteractionReranker(cfg)
    assert li.token_dtype == "res2" and li.codec_config == {"centroids": None, "train_docs": 4096, "kmeans_iters": 8, "codec_seed": 0}
    assert LateInteractionReranker({**cfg, "centroids": 64, "codec_seed": 3}).codec_config["centroids"] == 64
    for bad in ({"centroids": 48}, {"centroids": 8}, {"centroids": 1 << 21}, {"centroids": "64"}, {"train_docs": 0}, {"kmeans_iters": 0},
                {"codec_seed": -1}):
        with pytest.raises(ValueError, match=next(iter(bad))):
            LateInteractionReranker({**cfg, **bad})
    # the default count: the power of two nearest 16 sqrt(tokens), halved until the sample holds 32 tokens per centroid
    none = li.codec_config
    assert tc.resolve_centroids(none, 1 << 20, 1 << 30) == 1 << 14
    assert tc.resolve_centroids(none, 1 << 20, 32 * 1024) == 1024 and tc.resolve_centroids(none, 100, 10) == 16
    assert tc.index_bytes(1000, 128, 64) == 1000 * 38 + 64 * 256


def test_new_symbols_are_declared_exported_and_bound():
    import torch
    from rag import _native as nat
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crs_hip.h")).read(), flags=re.S)
    lib = nat.load()
    for name in ("crs_token_compress", "crs_maxsim_rc", "crs_maxsim_topk_rc", "crs_maxsim_topk_rc_workspace_bytes",
                 "crs_maxsim_topk_rc_plan_describe"):
        assert re.search(r"\bint %s\s*\(" % name, header) and hasattr(lib, name) and name in nat.exported_symbols(), name
    assert lib.crs_abi_version() == 3
    nat.ops()
    assert str(torch.ops.crs.maxsim_rc.default._schema) == \
        ("crs::maxsim_rc(Tensor q16, Tensor q_len, Tensor cid, Tensor codes, Tensor scale, Tensor centroids, Tensor weights, "
         "int n_tokens, Tensor offsets, int n_rows, Tensor rows, Tensor(a!) out) -> ()")
    assert hasattr(torch.ops.crs, "token_compress") and hasattr(torch.ops.crs, "maxsim_topk_rc")
