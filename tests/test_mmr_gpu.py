"""GPU: the MMR ordering kernel (csrc/mmr.hip, crs::mmr_order_out) against the fp64 restatement in tests/_mmr_ref.py, and the
retriever's opt-in mmr_vectors: 'device' path end to end.

The kernel's cosines are fp32, so its order may differ from the fp64 order where two candidates' values are closer than
eps = 2 (1 - lam) (dim + 8) 2^-24 (derived in _mmr_ref.py).  Every list must REPLAY: walking the device's order in fp64, each
pick is within eps of that round's best.  Lists whose fp64 margin is at least eps must match the fp64 order exactly."""
import numpy as np
import pytest

import _mmr_ref as ref

pytestmark = pytest.mark.gpu

N_ROWS, NQ = 4096, 256
# (dim, m_max, lam, generator, exact order required where the margin allows)
SHAPES = [(384, 10, 0.9, "random", True), (384, 20, 0.9, "cluster", True), (768, 20, 0.9, "cluster", True),
          (100, 33, 0.7, "cluster", True), (1024, 64, 0.5, "cluster", False), (1023, 64, 0.5, "cluster", False),
          (384, 2, 0.9, "random", False)]
MAX_EXCLUDED = 0.15


def _run(cuda, vecs, n_rows, rows, rel, counts, lam):
    """vecs: a cuda fp32 tensor (the caller may pass a view); the lists as numpy -> the order as numpy."""
    import torch
    from rag import _native as nat
    order = nat.mmr_order(vecs, n_rows, torch.from_numpy(rows).to(cuda), torch.from_numpy(rel).to(cuda),
                          torch.from_numpy(counts).to(cuda), lam)
    torch.cuda.synchronize()
    return order.cpu().numpy()


def _check_shape_of(order, counts, what):
    m_max = order.shape[1]
    for i, c in enumerate(counts.tolist()):
        assert sorted(order[i, :c].tolist()) == list(range(c)), f"{what}: list {i} is no permutation: {order[i]}"
        assert c == 0 or order[i, 0] == 0, f"{what}: list {i} does not start with position 0"
        assert (order[i, c:] == -1).all(), f"{what}: list {i} has entries past its count: {order[i]}"
    assert order.dtype == np.int32 and order.shape == (len(counts), m_max)


@pytest.mark.parametrize("dim,m_max,lam,kind,exact", SHAPES, ids=lambda v: str(v))
def test_op_matches_fp64(cuda, dim, m_max, lam, kind, exact):
    import torch
    case = ref.make_case(kind, dim, m_max, NQ, seed=dim * 100 + m_max, n_rows=N_ROWS)
    counts = case["counts"]
    assert {0, 1, min(2, m_max), m_max} <= set(counts.tolist())
    order = _run(cuda, torch.from_numpy(case["vecs"]).to(cuda), N_ROWS, case["rows"], case["rel"], counts, lam)
    what = f"dim {dim} m_max {m_max} lam {lam} {kind}"
    _check_shape_of(order, counts, what)
    eps = ref.eps_for(dim, lam)
    excluded, differ = 0, 0
    for i in range(NQ):
        v, rel = ref.list_of(case, i)
        got = order[i, :counts[i]].tolist()
        assert ref.replay_ok(got, v, rel, lam, eps), f"{what}: list {i} (count {counts[i]}) does not replay within eps {eps:.3e}: {got}"
        if exact:
            if ref.min_margin(v, rel, lam) >= eps:
                assert got == ref.mmr_order_ref(v, rel, lam), f"{what}: list {i} (count {counts[i]}) differs from the fp64 order"
            else:
                excluded += 1
        else:
            differ += got != ref.mmr_order_ref(v, rel, lam)
    print(f"{what}: eps {eps:.3e}, {excluded} of {NQ} lists under the margin, {differ} replay-only lists differ from the fp64 order")
    if exact:
        assert excluded <= MAX_EXCLUDED * NQ, f"{what}: {excluded} of {NQ} lists excluded by the margin rule"


def test_ties_go_to_the_lower_position_and_runs_repeat(cuda):
    import torch
    rng = np.random.default_rng(7)
    dim, m_max, lam = 384, 12, 0.8
    base = rng.standard_normal((16, dim))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    vecs = base.astype(np.float32)
    # list 0: rows 1 and 2 are the same row (3), as are 4 and 5 (7), with equal rel each; list 1: 12 times one row, rel descending
    rows = np.array([[0, 3, 3, 5, 7, 7, 9, 11, 2, 4, 6, 8], [13] * 12], dtype=np.int64)
    rel = np.array([[0.9, 0.8, 0.8, 0.7, 0.6, 0.6, 0.5, 0.45, 0.4, 0.35, 0.3, 0.25],
                    list(np.linspace(0.9, 0.35, 12))], dtype=np.float64)
    counts = np.array([12, 12], dtype=np.int32)
    dev = torch.from_numpy(vecs).to(cuda)
    first = _run(cuda, dev, 16, rows, rel, counts, lam)
    _check_shape_of(first, counts, "ties")
    got = first[0].tolist()
    assert got.index(1) < got.index(2) and got.index(4) < got.index(5), f"duplicates out of position order: {got}"
    assert got == ref.mmr_order_ref(vecs[rows[0]].astype(np.float64), rel[0], lam)
    assert first[1].tolist() == list(range(12)), f"identical rows with descending rel: {first[1]}"
    again = _run(cuda, dev, 16, rows, rel, counts, lam)
    assert first.tobytes() == again.tobytes()


def test_ids_outside_the_shard_are_zero_vectors_not_addresses(cuda):
    """vecs is a view 8 rows inside a larger tensor and n_rows is 8 short of what remains, so an id that the kernel failed to
    refuse reads other rows of the same allocation: a wrong answer here, not a fault."""
    import torch
    dim, m_max, lam, nq = 100, 16, 0.7, 64
    total = 512
    n_rows = total - 8 - 8
    case = ref.make_case("cluster", dim, m_max, nq, seed=11, n_rows=total)
    rng = np.random.default_rng(12)
    case["rows"] = np.where(case["rows"] >= 0, case["rows"] % n_rows, -1)
    case["vecs"][8 + 5] = 0.0                                  # a zero row, listed below
    for i in range(nq):
        c = int(case["counts"][i])
        if c >= 3:
            at = rng.choice(np.arange(1, c), size=min(3, c - 1), replace=False)
            for a, bad in zip(at, (-1, n_rows, n_rows + 3)):
                case["rows"][i, a] = bad
        if c >= 6:
            case["rows"][i, 5] = 5                             # the zero row
    whole = torch.from_numpy(case["vecs"]).to(cuda)
    order = _run(cuda, whole[8:], n_rows, case["rows"], case["rel"], case["counts"], lam)
    _check_shape_of(order, case["counts"], "poisoned ids")
    eps = ref.eps_for(dim, lam)
    for i in range(nq):
        v, rel = ref.list_of(case, i, n_rows=n_rows, base=8)
        got = order[i, :case["counts"][i]].tolist()
        assert ref.replay_ok(got, v, rel, lam, eps), f"list {i}: {got}"
        if ref.min_margin(v, rel, lam) >= eps:
            assert got == ref.mmr_order_ref(v, rel, lam), f"list {i}: {got}"


# ---- end to end ---------------------------------------------------------------------------------------------------------------
WORDS = ("retrieval augmented generation language model quantization weights perplexity attention embedding cosine "
         "similarity vector index chunk context answer question compression memory latency throughput").split()
E2E_ROWS, E2E_DIM, E2E_Q = 4096, 384, 128


def _pipeline(cuda, refine_fp32=True):
    import torch
    from rag import RAGPipeline
    from rag.chunking import Chunk

    class Stub:
        def generate(self, prompt, **kw):
            return "n/a"

    cfg = {"embedding": {"model_name": "synthetic:minilm", "device": "cuda", "batch_size": 64, "normalize": True},
           "retrieval": {"top_k": 10, "similarity_threshold": 0.0, "rerank": True, "diversity_penalty": 0.1, "batch_queries": 64,
                         "mmr_vectors": "device"},
           "vector_store": {"collection_name": f"mmr-e2e-{int(refine_fp32)}", "refine_fp32": refine_fp32}}
    p = RAGPipeline(cfg)
    p.setup(Stub())
    rng = np.random.default_rng(21)
    chunks = [Chunk(text=" ".join(rng.choice(WORDS, size=6)) + f" {r}", chunk_id=f"c_{r}", start_char=0, end_char=1, page_number=None)
              for r in range(E2E_ROWS)]
    g = torch.Generator(device=cuda); g.manual_seed(22)
    centres = torch.randn((E2E_ROWS // 8, E2E_DIM), generator=g, device=cuda).repeat_interleave(8, dim=0)
    p.vector_store.create_index(chunks, centres + 0.3 * torch.randn((E2E_ROWS, E2E_DIM), generator=g, device=cuda))
    questions = [" ".join(rng.choice(WORDS, size=int(rng.integers(4, 9)))) + f" {q}" for q in range(E2E_Q)]
    return p, questions


@pytest.fixture(scope="module")
def e2e(cuda):
    return _pipeline(cuda)


def _both(p, questions, top_k=None):
    r = p.retriever
    out = {}
    for mode in ("index", "device"):
        r.mmr_vectors = mode
        out[mode] = (p.retrieve_batch(questions, top_k=top_k), dict(r.last_mmr))
    r.mmr_vectors = "device"
    return out


def _replays(p, lists, penalty):
    store = p.vector_store
    row = {cid: r for r, cid in enumerate(store.collection.ids)}
    lam = 1.0 - penalty
    eps = ref.eps_for(E2E_DIM, lam)
    for a, chunks in enumerate(lists):
        if len(chunks) > 1:
            v = store.rows_f32([row[c["chunk_id"]] for c in chunks]).astype(np.float64)
            assert ref.replay_ok(list(range(len(chunks))), v, [c["score"] for c in chunks], lam, eps), f"query {a} does not replay"


@pytest.mark.parametrize("penalty", [0.1, 0.5])
def test_retrieve_batch_on_device_returns_the_host_chunks_in_an_mmr_order(cuda, e2e, penalty):
    p, questions = e2e
    p.retriever.diversity_penalty = penalty
    both = _both(p, questions)
    (host, host_info), (dev, dev_info) = both["index"], both["device"]
    assert dev_info["mode"] == "device" and dev_info["lists"] == sum(len(c) > 1 for c in dev), dev_info
    assert host_info["mode"] == "host", host_info
    assert sum(len(c) > 1 for c in dev) >= E2E_Q // 2
    for a in range(E2E_Q):
        by_id = {c["chunk_id"]: c for c in host[a]}
        assert {c["chunk_id"] for c in dev[a]} == set(by_id), f"query {a}: other chunks"
        assert len(dev[a]) == len(host[a])
        for c in dev[a]:
            assert c == by_id[c["chunk_id"]], f"query {a}: chunk {c['chunk_id']} differs"
        if host[a]:
            assert dev[a][0]["chunk_id"] == host[a][0]["chunk_id"]
    _replays(p, dev, penalty)
    one = p.retrieve(questions[3])
    assert one == p.retrieve_batch([questions[3]])[0]
    assert [c["chunk_id"] for c in one] == [c["chunk_id"] for c in dev[3]]
    p.retriever.diversity_penalty = 0.1


def test_lists_of_40_run_on_device_and_lists_of_80_on_the_host(cuda, e2e):
    p, questions = e2e
    r = p.retriever
    r.rerank, r.diversity_penalty = False, 0.1
    try:
        both = _both(p, questions, top_k=40)
        dev, info = both["device"]
        assert info == {"mode": "device", "lists": E2E_Q} and all(len(c) == 40 for c in dev)
        for a in range(E2E_Q):
            assert sorted(c["chunk_id"] for c in dev[a]) == sorted(c["chunk_id"] for c in both["index"][0][a])
        _replays(p, dev, 0.1)
        both = _both(p, questions[:64], top_k=80)
        dev, info = both["device"]
        assert info == {"mode": "host", "lists": 64} and all(len(c) == 80 for c in dev)
        assert dev == both["index"][0]
    finally:
        r.rerank = True


def test_store_without_fp32_rows_takes_the_host_path(cuda):
    p, questions = _pipeline(cuda, refine_fp32=False)
    r = p.retriever
    assert p.vector_store.mmr_order(np.zeros((1, 2), dtype=np.int64), np.zeros((1, 2)), np.array([2], dtype=np.int32), 0.9) is None
    dev = p.retrieve_batch(questions[:64])
    assert r.last_mmr["mode"] == "host" and r.last_mmr["lists"] == sum(len(c) > 1 for c in dev)
    r.mmr_vectors = "auto"
    assert p.retrieve_batch(questions[:64]) == dev
