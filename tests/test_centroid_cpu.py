"""CPU: the pruned centroid sweep's plan as a pure function, the retriever's first_stage 'centroid' keys, and the new
symbols."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVES = 16      # kCsWaves: every wave of a workgroup walks items of its own


def _plan(nq, n_centroids, row_count=1000000, lq_max=32, k=10):
    from rag import _native as nat
    line = nat.centroid_maxsim_topk_plan_describe(nq, lq_max, n_centroids, k, row_count)
    m = re.search(r"centroid_scan<ch=(\d+)> grid=(\d+)x(\d+) threads=1024 Qg=(\d+) bitmap_words=(\d+) lqp=(\d+) .*kp=(\d+) lds=(\d+)", line)
    return dict(zip(("ch", "g", "qgroups", "qg", "words", "lqp", "kp", "lds"), (int(x) for x in m.groups())))


@pytest.mark.parametrize("n_centroids, qg", [(16, 8), (1 << 17, 8), ((1 << 17) + 32, 7), (1 << 18, 4), (1 << 19, 2), (1 << 20, 1)])
def test_queries_of_a_workgroup_follow_the_bitmap(n_centroids, qg):
    """Qg = min(8, 128 KB / bitmap bytes); the grid at nq = Qg and Qg + 1; LDS holds the bitmaps or the final lists."""
    p = _plan(qg, n_centroids)
    assert (p["qg"], p["qgroups"], p["words"]) == (qg, 1, -(-n_centroids // 32))
    assert p["lds"] == max(qg * p["words"] * 4, qg * WAVES * 64 * 8) <= 128 * 1024
    assert p["g"] == 256
    more = _plan(qg + 1, n_centroids)
    assert (more["qgroups"], more["g"]) == (2, 128)
    assert _plan(1, n_centroids, row_count=64 * WAVES + 1)["g"] == 2      # one item per wave, and one more


@pytest.mark.parametrize("lq_max, lqp, ch", [(1, 8, 1), (9, 16, 2), (17, 24, 4), (32, 32, 4), (33, 40, 8), (64, 64, 8)])
def test_score_rows_are_cut_into_16_byte_chunks(lq_max, lqp, ch):
    p = _plan(3, 1024, lq_max=lq_max, k=33)
    assert (p["lqp"], p["ch"], p["kp"]) == (lqp, ch, 64)


def test_workspace_bound_grows_with_its_arguments():
    from rag import _native as nat
    ws = nat.centroid_maxsim_topk_workspace_bytes
    for nq in (1, 8, 9, 300):
        p = _plan(nq, 1 << 17)
        assert ws(nq, 10, 1000000) >= p["g"] * nq * p["kp"] * 12
    assert ws(1, 10, 64) <= ws(2, 10, 64) <= ws(2, 33, 64) <= ws(2, 33, 6400) <= ws(2, 33, 1 << 30)
    for bad, word in (((1, 65, 10), "k must"), ((1, 1, 2 ** 32), "row_count"), ((65536, 1, 10), "nq")):
        with pytest.raises(nat.NativeError, match=word):
            ws(*bad)
    with pytest.raises(nat.NativeError, match="n_centroids"):
        nat.centroid_maxsim_topk_plan_describe(1, 32, 15, 10, 100)


def test_the_centroid_first_stage_keys_are_validated():
    from rag.retrieval import ContextRetriever

    class Store:
        def token_index(self):
            raise AssertionError("not built at construction")

        def attach_token_encoder(self, encoder):
            self.encoder = encoder

    base = {"model_name": "synthetic:tiny-colbert", "token_dtype": "res2", "first_stage": "centroid"}
    make = lambda li: ContextRetriever(Store(), None, {"late_interaction": li, "top_k": 5})
    r = make(base)
    assert (r.late_first_stage, r.centroid_threshold, r.centroid_candidates) == ("centroid", 0.5, 64)
    r = make({**base, "centroid_threshold": 0.25, "centroid_candidates": 10})
    assert (r.centroid_threshold, r.centroid_candidates) == (0.25, 10)
    assert sorted(r.late_interaction.codec_config) == ["centroids", "codec_seed", "kmeans_iters", "train_docs"]
    for bad, word in (({"token_dtype": "fp16"}, "token_dtype"), ({"token_dtype": "fp8"}, "token_dtype"), ({"first_stage": "plaid"}, "first_stage"),
                      ({"centroid_threshold": "0.5"}, "centroid_threshold"), ({"centroid_threshold": float("nan")}, "centroid_threshold"),
                      ({"centroid_candidates": 65}, "centroid_candidates"), ({"centroid_candidates": 0}, "centroid_candidates"),
                      ({"centroid_candidates": 8.0}, "centroid_candidates")):
        with pytest.raises(ValueError, match=word):
            make({**base, **bad})


def test_new_symbols_are_declared_exported_and_bound():
    import torch
    from rag import _native as nat
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crs_hip.h")).read(), flags=re.S)
    lib = nat.load()
    for name in ("crs_centroid_scores", "crs_centroid_maxsim_topk", "crs_centroid_maxsim_topk_workspace_bytes",
                 "crs_centroid_maxsim_topk_plan_describe"):
        assert re.search(r"\bint %s\s*\(" % name, header) and hasattr(lib, name) and name in nat.exported_symbols(), name
    nat.ops()
    assert str(torch.ops.crs.centroid_scores.default._schema) == \
        "crs::centroid_scores(Tensor q16, Tensor q_len, Tensor centroids, float threshold, Tensor(a!) s16, Tensor(b!) keep) -> ()"
    assert hasattr(torch.ops.crs, "centroid_maxsim_topk")
