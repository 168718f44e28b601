"""GPU: crs::merge_sorted / crs::merge_sorted_wire (csrc/merge_sorted.hip) -- the co-ranking merge of sorted top-k lists that
serves top_k 65 .. 1024 on sharded stores.

The kernel does no arithmetic, so every check is byte equality (scores as int32, ids) against a reference stated here: numpy
lexsort of the valid entries by (score desc, id asc), truncated to k_out and padded with (-inf, -1).  The same data goes
through the separate-array front end and the wire front end, and through VectorStore._order, the path the kernel replaces."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (nlists, nq, k_in, k_out): one list (copy), the smallest k above merge_topk's 64, more queries than a wave, k_out < k_in,
# k_out > k_in, the largest lists (two LDS groups), the most lists (64 x 64 -> k_out 1024), k_in that is no power of two
SHAPES = [(1, 3, 100, 100), (2, 1, 65, 65), (2, 70, 100, 100), (3, 5, 100, 37), (3, 5, 40, 100), (8, 4, 1024, 1024),
          (64, 2, 64, 1024), (5, 2, 1000, 1024)]
CONTENTS = ["random", "equal", "seven", "last_list", "padded", "all_empty", "few"]


def make_lists(content, nlists, nq, k_in, k_out, seed, pad_score=None):
    """scores fp32 / ids int64 [nlists, nq, k_in], every list sorted (score desc, id asc) with its empty slots at the tail; ids >= 0
    distinct across the lists of a query.  pad_score: the score bits of empty slots (None: garbage the kernel must ignore)."""
    rng = np.random.default_rng(seed)
    s = np.empty((nlists, nq, k_in), dtype=np.float32)
    i = np.empty((nlists, nq, k_in), dtype=np.int64)
    for q in range(nq):
        pool = rng.permutation(3 * nlists * k_in + 7)[: nlists * k_in].reshape(nlists, k_in).astype(np.int64)
        for l in range(nlists):
            if content == "equal":
                sc = np.full(k_in, 0.25, dtype=np.float32)
            elif content == "seven":
                sc = rng.choice(np.linspace(-1, 1, 7).astype(np.float32), size=k_in)
            else:
                sc = rng.standard_normal(k_in).astype(np.float32)
            if content == "last_list" and l == nlists - 1:
                sc = sc + np.float32(10.0)
            valid = k_in
            if content == "padded":
                valid = int(rng.integers(0, k_in + 1))
                if (l == 0 and q == 0) or (q == nq - 1 and nq > 1):
                    valid = 0                                   # a wholly empty list; the last query: every list empty
            elif content == "all_empty":
                valid = 0
            elif content == "few":
                valid = min(k_in, (k_out - 1) // nlists)        # nlists * valid < k_out
            ids = pool[l]
            o = np.lexsort((ids[:valid], -sc[:valid]))
            s[l, q, :valid], i[l, q, :valid] = sc[:valid][o], ids[:valid][o]
            s[l, q, valid:] = rng.standard_normal(k_in - valid).astype(np.float32) + 3 if pad_score is None else pad_score
            i[l, q, valid:] = -1
    return s, i


def reference(s, i, k_out):
    nlists, nq, k_in = s.shape
    out_s = np.full((nq, k_out), -np.inf, dtype=np.float32)
    out_i = np.full((nq, k_out), -1, dtype=np.int64)
    for q in range(nq):
        sq, iq = s[:, q].reshape(-1), i[:, q].reshape(-1)
        sq, iq = sq[iq >= 0], iq[iq >= 0]
        o = np.lexsort((iq, -sq))[:k_out]
        out_s[q, : len(o)], out_i[q, : len(o)] = sq[o], iq[o]
    return out_s, out_i


def same_bytes(got_s, got_i, want_s, want_i, what):
    got_s, got_i = got_s.cpu().numpy(), got_i.cpu().numpy()
    assert np.array_equal(got_i, want_i), f"{what}: ids differ at {np.argwhere(got_i != want_i)[:5].tolist()}"
    assert np.array_equal(got_s.view(np.int32), want_s.view(np.int32)), f"{what}: score bits differ"


def pack(cuda, s, i):
    import torch
    from rag import _shard
    return torch.cat([_shard.pack_wire(torch.from_numpy(s[l]), torch.from_numpy(i[l])) for l in range(s.shape[0])]).to(cuda)


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda t: "x".join(map(str, t)))
def test_both_front_ends_equal_the_lexsort_reference(cuda, shape, content):
    import torch
    from rag import _native as nat
    nlists, nq, k_in, k_out = shape
    s, i = make_lists(content, nlists, nq, k_in, k_out, seed=10 * SHAPES.index(shape) + CONTENTS.index(content))
    want_s, want_i = reference(s, i, k_out)
    if content == "few":
        assert (want_i[:, -1] == -1).all()
    got_s, got_i = nat.merge_sorted(torch.from_numpy(s).to(cuda), torch.from_numpy(i).to(cuda), k_out)
    same_bytes(got_s, got_i, want_s, want_i, f"{shape} {content} arrays")
    out_s = torch.full((nq, k_out), float("nan"), dtype=torch.float32, device=cuda)
    out_i = torch.full((nq, k_out), -7, dtype=torch.int64, device=cuda)
    nat.merge_sorted_wire(pack(cuda, s, i), nlists, nq, k_in, k_out, out_scores=out_s, out_ids=out_i)
    same_bytes(out_s, out_i, want_s, want_i, f"{shape} {content} wire")


def test_wire_layout_at_1024():
    from rag import _native as nat, _shard
    lib = nat.load()
    for nq in (1, 3, 64):
        assert (lib.crs_wire_bytes(nq, 1024), lib.crs_wire_scores_offset(nq, 1024)) == _shard.wire_layout(nq, 1024)
        assert (lib.crs_wire_bytes(nq, 65), lib.crs_wire_scores_offset(nq, 65)) == _shard.wire_layout(nq, 65)


@pytest.mark.parametrize("content", ["random", "seven", "padded", "few"])
@pytest.mark.parametrize("shape", [(2, 70, 100, 100), (3, 5, 40, 100), (8, 4, 1024, 1024), (64, 2, 64, 1024)], ids=lambda t: "x".join(map(str, t)))
def test_equals_the_two_stable_sorts_it_replaces(cuda, shape, content):
    """VectorStore._order on the stacked lists, as _topk_device called it before the kernel (empty slots carry -inf as the shards
    write them)"""
    import torch
    from rag import _native as nat
    from rag.indexing import VectorStore
    nlists, nq, k_in, k_out = shape
    s, i = make_lists(content, nlists, nq, k_in, k_out, seed=5 + nlists, pad_score=-np.inf)
    gs, gi = torch.from_numpy(s).to(cuda), torch.from_numpy(i).to(cuda)
    want_s, want_i = VectorStore._order(gs.permute(1, 0, 2).reshape(nq, -1), gi.permute(1, 0, 2).reshape(nq, -1), k_out)
    if want_s.shape[1] < k_out:          # _order keeps what there is; the store's callers never ask for more
        pad = k_out - want_s.shape[1]
        want_s = torch.nn.functional.pad(want_s, (0, pad), value=float("-inf"))
        want_i = torch.nn.functional.pad(want_i, (0, pad), value=-1)
    got_s, got_i = nat.merge_sorted(gs, gi, k_out)
    same_bytes(got_s, got_i, want_s.cpu().numpy(), want_i.cpu().numpy(), f"{shape} {content} vs _order")


def test_argument_errors_are_host_side(cuda):
    import torch
    from rag import _native as nat

    def lists(nlists, k=8):
        return (torch.zeros((nlists, 2, k), dtype=torch.float32, device=cuda), torch.full((nlists, 2, k), -1, dtype=torch.int64, device=cuda))
    with pytest.raises(nat.NativeError):
        nat.merge_sorted(*lists(2), 1025)
    with pytest.raises(nat.NativeError):
        nat.merge_sorted(*lists(65), 8)
    with pytest.raises(nat.NativeError):
        nat.merge_sorted(*lists(0), 8)
    with pytest.raises(nat.NativeError):
        nat.merge_sorted(*lists(2, 1025), 8)
    wire = torch.zeros(2 * nat.load().crs_wire_bytes(2, 8), dtype=torch.uint8, device=cuda)
    for nl, k_out in ((2, 1025), (65, 8), (0, 8)):
        with pytest.raises(nat.NativeError):
            nat.merge_sorted_wire(wire, nl, 2, 8, k_out)
    with pytest.raises(nat.NativeError, match="CRS_MAX_K"):        # the old entry point keeps its limit
        nat.merge_topk(*lists(2, 100), 100)
    with pytest.raises(nat.NativeError, match="CRS_MAX_K"):
        nat.merge_topk_wire(wire, 2, 2, 8, 100)
    torch.cuda.synchronize()


def test_graph_replay_holds_no_state(cuda):
    import torch
    from rag import _native as nat
    nlists, nq, k_in, k_out = 8, 4, 1024, 1024
    s, i = make_lists("seven", nlists, nq, k_in, k_out, seed=31)
    gs, gi = torch.from_numpy(s).to(cuda), torch.from_numpy(i).to(cuda)
    out_s = torch.empty((nq, k_out), dtype=torch.float32, device=cuda)
    out_i = torch.empty((nq, k_out), dtype=torch.int64, device=cuda)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        nat.merge_sorted(gs, gi, k_out, out_s, out_i)
    torch.cuda.current_stream().wait_stream(st)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        nat.merge_sorted(gs, gi, k_out, out_s, out_i)
    want = reference(s, i, k_out)
    for _ in range(2):
        out_s.fill_(float("nan"))
        out_i.fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
        same_bytes(out_s, out_i, *want, "replay")
    s2, i2 = make_lists("padded", nlists, nq, k_in, k_out, seed=32)      # new inputs in the captured buffers
    gs.copy_(torch.from_numpy(s2))
    gi.copy_(torch.from_numpy(i2))
    graph.replay()
    torch.cuda.synchronize()
    same_bytes(out_s, out_i, *reference(s2, i2, k_out), "replay on new inputs")
