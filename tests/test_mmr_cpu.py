"""CPU: the MMR ordering entry point (crs_mmr_order, csrc/mmr.hip) is declared, exported and bound, the ABI version did not move,
its argument checks answer CRS_EINVAL before any HIP call, its kernel uses no scratch; the retriever accepts
mmr_vectors: 'device'; the _rerank token-set cache changes no value."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_exported_and_bound():
    import torch
    from rag import _native as nat
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crs_hip.h")).read(), flags=re.S)
    lib = nat.load()
    assert re.search(r"\bint crs_mmr_order\s*\(", header), "crs_mmr_order not declared in include/crs_hip.h"
    assert hasattr(lib, "crs_mmr_order"), "crs_mmr_order not exported"
    assert "crs_mmr_order" in nat.exported_symbols()
    assert lib.crs_abi_version() == 3
    # the binding table still names exactly the functions of the header
    declared = set(re.findall(r"\b(crs_\w+)\s*\(", header))
    assert set(nat._SIGNATURES) & declared == declared, sorted(declared - set(nat._SIGNATURES))
    assert hasattr(nat.ops(), "mmr_order_out") and callable(nat.mmr_order)
    assert str(torch.ops.crs.mmr_order_out.default._schema) == \
        "crs::mmr_order_out(Tensor vecs, int n_rows, Tensor rows, Tensor rel, Tensor counts, float lam, Tensor(a!) order) -> ()"


def test_argument_validation_without_gpu():
    from rag import _native as nat
    lib = nat.load()
    buf = (ctypes.c_char * 4096)()                     # host memory standing in for device pointers: never dereferenced
    p = ctypes.cast(buf, ctypes.c_void_p)
    EINVAL = -1

    # crs_mmr_order(vecs, n_rows, dim, rows, rel, counts, nq, m_max, lam, order, stream)
    def call(vecs=p, n_rows=100, dim=384, rows=p, rel=p, counts=p, nq=4, m_max=10, lam=0.9, order=p):
        return lib.crs_mmr_order(vecs, n_rows, dim, rows, rel, counts, nq, m_max, lam, order, None)

    for bad, word in (({"nq": -1}, b"nq"), ({"dim": 0}, b"dim"), ({"dim": -3}, b"dim"), ({"m_max": 0}, b"m_max"), ({"m_max": 65}, b"m_max"),
                      ({"m_max": -1}, b"m_max"), ({"lam": -0.01}, b"lam"), ({"lam": 1.01}, b"lam"), ({"lam": float("nan")}, b"lam"),
                      ({"vecs": None}, b"null pointer"), ({"rows": None}, b"null pointer"), ({"rel": None}, b"null pointer"),
                      ({"counts": None}, b"null pointer"), ({"order": None}, b"null pointer")):
        assert call(**bad) == EINVAL, bad
        assert word in lib.crs_last_error(), (bad, lib.crs_last_error())
    assert call(nq=0) == 0                             # nothing to order: no launch


def test_kernel_uses_no_scratch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_resources.py"), "mmr.hip"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "0 violation(s)" in r.stdout and "1 kernels in 1 files" in r.stdout, r.stdout


class _Store:
    collection = None


def test_retriever_accepts_device_and_rejects_unknown_values():
    from rag.retrieval import ContextRetriever
    r = ContextRetriever(_Store(), None, {"mmr_vectors": "device"})
    assert r.mmr_vectors == "device" and r.last_mmr == {"mode": "host", "lists": 0}
    for mode in ("auto", "reembed", "index"):
        assert ContextRetriever(_Store(), None, {"mmr_vectors": mode}).mmr_vectors == mode
    with pytest.raises(ValueError, match="'device'"):
        ContextRetriever(_Store(), None, {"mmr_vectors": "gpu"})


def _uncached_rerank(query, chunks, top_k):
    """_rerank as it was before the cache: the token set rebuilt for every hit."""
    wanted = set(query.lower().split())
    norm = max(len(wanted), 1)
    for chunk in chunks:
        hits = len(wanted & set(chunk['text'].lower().split()))
        chunk['rerank_score'] = chunk['score'] * 0.7 + (hits / norm) * 0.3
    chunks.sort(key=lambda c: c.get('rerank_score', c['score']), reverse=True)
    return chunks[:top_k]


def test_rerank_token_cache_changes_no_value():
    import copy
    import random
    from rag.retrieval import ContextRetriever
    rnd = random.Random(5)
    words = "Alpha beta GAMMA delta epsilon zeta eta theta iota kappa".split()
    texts = [" ".join(rnd.choice(words) for _ in range(rnd.randint(0, 8))) for _ in range(40)] + ["", "  tab\tseparated\nWords  "]
    r = ContextRetriever(_Store(), None, {"rerank": True})
    for round_ in range(3):                             # the same texts again (cache hits), then changed texts under the same ids
        if round_ == 2:
            texts = [t + " kappa" for t in texts]
        for q in ("alpha BETA", "theta theta iota", "", "nothing here"):
            chunks = [{"text": t, "score": rnd.random(), "chunk_id": f"c{i}"} for i, t in enumerate(texts)]
            want = _uncached_rerank(q, copy.deepcopy(chunks), 7)
            assert r._rerank(q, copy.deepcopy(chunks), 7) == want
    assert 0 < len(r._token_sets) <= r.TOKEN_SET_CACHE_CAP
    # the cap: the cache is dropped when it is full, and answers stay the same
    r.TOKEN_SET_CACHE_CAP = 8
    chunks = [{"text": t + " zeta", "score": 0.5, "chunk_id": f"c{i}"} for i, t in enumerate(texts)]     # texts not cached yet
    assert r._rerank("alpha", copy.deepcopy(chunks), 5) == _uncached_rerank("alpha", copy.deepcopy(chunks), 5)
    assert len(r._token_sets) <= 8
