"""GPU: the BERTScore matching kernel (csrc/token_match.hip, crs::token_match_out) against fp64 numpy over the same fp32
token states; BertScorer end to end against tests/golden/bertscore.npz (transformers in fp64); the scorer's batching.

Bound on P and R of the kernel alone, in units of u = 2^-24, with S the longer side:  (2 H + S + 32) u.
  * a dot product is an fmaf chain of H terms (the f32-input MFMA, in a fixed permutation of k -- any order has the same
    bound): |error| <= gamma_H sum |a_k b_k| <= H u |a| |b| by Cauchy-Schwarz, i.e. H u on the cosine's scale;
  * each sum of squares is a chain of H / 16 fmafs per lane plus a 4-step butterfly, relative error <= (H / 16 + 4) u, halved
    by the square root; 1 / sqrt adds 2 u per side and the two products by the inverse norms 2 u: below (H + 8) u in all;
  * a maximum moves by no more than its arguments do;
  * the weighted mean adds at most S / 64 + 6 fmaf / add roundings per sum on values <= 1 and one division: below (S + 2) u.
The remaining 22 u are slack; the worst error measured on an MI355X is 8.2e-07 (H 1024, 5 x 130; bound 1.3e-04), each test
prints its own beside the bound.  F is checked against fp32(2 P R / (P + R)) of the RETURNED P and R: two products and a
division, 4 ulp."""
import numpy as np
import pytest

import _bertscore_cases as bc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def bound(hidden, seq_a, seq_b):
    return (2 * hidden + max(seq_a, seq_b) + 32) * U


def _run(cuda, a, la, b, lb, wa=None, wb=None):
    import torch
    from rag import _native as nat
    t = lambda x, dt: None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(cuda)
    out = nat.token_match(t(a, np.float32), t(la, np.int32), t(b, np.float32), t(lb, np.int32), t(wa, np.float32), t(wb, np.float32))
    torch.cuda.synchronize()
    assert out.shape == (a.shape[0], 3) and out.dtype == torch.float32
    return out.cpu().numpy()


def _lens(seq, reverse=False):
    """1, seq, and values that are no multiple of 16 (where seq allows)."""
    ls = [seq, 1, max(1, seq - 3), max(1, (2 * seq) // 3) | 1, seq // 2 + 1]
    ls = [min(max(1, v), seq) for v in ls]
    return np.asarray(ls[::-1] if reverse else ls, dtype=np.int32)


def _states(rng, n, seq_a, seq_b, hidden, la, lb):
    """Candidates ~N(0, 1) per element with per-row scales over 3 decades; half of a reference's rows are noisy copies of
    candidate rows, the others independent."""
    a = rng.standard_normal((n, seq_a, hidden)).astype(np.float32) * np.exp(rng.uniform(-3, 3, (n, seq_a, 1))).astype(np.float32)
    b = rng.standard_normal((n, seq_b, hidden)).astype(np.float32)
    for p in range(n):
        for j in range(int(lb[p])):
            if rng.random() < 0.5:
                i = rng.integers(0, int(la[p]))
                b[p, j] = a[p, i] / np.linalg.norm(a[p, i]) * np.sqrt(hidden) + 0.7 * b[p, j]
    return a, b


def _check_f(out):
    P, R, F = out[:, 0].astype(np.float64), out[:, 1].astype(np.float64), out[:, 2]
    for p in range(out.shape[0]):
        s = np.float32(P[p]) + np.float32(R[p])
        if s == 0 or not np.isfinite(s):
            assert F[p] == 0, (p, out[p])
        else:
            want = np.float32(2 * P[p] * R[p] / (P[p] + R[p]))
            assert abs(float(F[p]) - float(want)) <= 4 * np.spacing(np.abs(want)), (p, out[p], want)


@pytest.mark.parametrize("seq_a,seq_b", [(1, 1), (5, 130), (17, 33), (100, 64), (512, 512)], ids=lambda v: str(v))
@pytest.mark.parametrize("hidden", [64, 384, 768, 1024])
def test_kernel_matches_fp64(cuda, hidden, seq_a, seq_b):
    rng = np.random.default_rng(hidden * 1000 + seq_a)
    la, lb = _lens(seq_a), _lens(seq_b, reverse=True)
    n = len(la)
    a, b = _states(rng, n, seq_a, seq_b, hidden, la, lb)
    wa = rng.uniform(0.0, 3.0, (n, seq_a)).astype(np.float32)
    wb = rng.uniform(0.0, 3.0, (n, seq_b)).astype(np.float32)
    tol = bound(hidden, seq_a, seq_b)
    for w1, w2 in ((None, None), (wa, wb)):
        out = _run(cuda, a, la, b, lb, w1, w2)
        want = bc.match_ref(a, la, b, lb, w1, w2)
        assert np.isfinite(out).all()
        err = np.abs(out[:, :2] - want[:, :2]).max()
        print(f"token_match H {hidden} {seq_a} x {seq_b} weights {w1 is not None}: max |P, R error| {err:.3e}  bound {tol:.3e}")
        assert err <= tol, (err, tol)
        _check_f(out)


def test_recall_exceeds_precision_when_the_reference_is_a_subset(cuda):
    """b = noisy copies of 40 of a's 100 rows: every reference token has a close candidate token (R high), most candidate
    tokens have none (P low).  Swapping a and b, or rows and columns, swaps the two."""
    rng = np.random.default_rng(5)
    hidden, seq_a, seq_b = 384, 100, 64
    la, lb = np.asarray([100, 77], dtype=np.int32), np.asarray([40, 23], dtype=np.int32)
    a = rng.standard_normal((2, seq_a, hidden)).astype(np.float32)
    b = rng.standard_normal((2, seq_b, hidden)).astype(np.float32)
    for p in range(2):
        pick = rng.permutation(int(la[p]))[: int(lb[p])]
        b[p, : lb[p]] = a[p, pick] + 0.3 * b[p, : lb[p]]
    out = _run(cuda, a, la, b, lb)
    want = bc.match_ref(a, la, b, lb)
    assert (want[:, 1] - want[:, 0] >= 0.05).all(), want
    assert (out[:, 1] - out[:, 0] >= 0.05).all(), out
    assert np.abs(out[:, :2] - want[:, :2]).max() <= bound(hidden, seq_a, seq_b)
    swapped = _run(cuda, b, lb, a, la)
    assert np.abs(swapped[:, 0] - out[:, 1]).max() <= 2 * bound(hidden, seq_a, seq_b)
    assert np.abs(swapped[:, 1] - out[:, 0]).max() <= 2 * bound(hidden, seq_a, seq_b)


def test_padding_is_never_read_into_a_result(cuda):
    rng = np.random.default_rng(6)
    hidden, seq_a, seq_b = 384, 70, 33
    la, lb = np.asarray([70, 1, 37, 64, 65], dtype=np.int32), np.asarray([17, 33, 1, 16, 32], dtype=np.int32)
    n = len(la)
    a, b = _states(rng, n, seq_a, seq_b, hidden, la, lb)
    wa, wb = rng.uniform(0.5, 2.0, (n, seq_a)).astype(np.float32), rng.uniform(0.5, 2.0, (n, seq_b)).astype(np.float32)
    outs = []
    for fill in ("poison", "zero"):
        a2, b2, wa2, wb2 = a.copy(), b.copy(), wa.copy(), wb.copy()
        for p in range(n):
            for x, w, ln in ((a2, wa2, la), (b2, wb2, lb)):
                x[p, ln[p]:] = 0.0
                w[p, ln[p]:] = 0.0
                if fill == "poison":
                    x[p, ln[p]::2] = np.nan
                    x[p, ln[p] + 1::2] = 1e30
                    w[p, ln[p]:] = np.nan
        outs.append(_run(cuda, a2, la, b2, lb, wa2, wb2))
    assert np.isfinite(outs[0]).all() and np.isfinite(outs[1]).all()
    assert outs[0].tobytes() == outs[1].tobytes()
    assert np.abs(outs[0][:, :2] - bc.match_ref(a, la, b, lb, wa, wb)[:, :2]).max() <= bound(hidden, seq_a, seq_b)


def test_a_pair_does_not_depend_on_its_launch(cuda):
    rng = np.random.default_rng(7)
    hidden, seq = 768, 33
    la, lb = _lens(seq)[[2, 0, 3, 4, 1, 0, 2]], _lens(seq)[[0, 3, 2, 1, 4, 4, 3]]       # 7 pairs; pair 2 is the one watched
    a, b = _states(rng, 7, seq, seq, hidden, la, lb)
    w = rng.uniform(0.5, 2.0, (7, seq)).astype(np.float32)
    batch = _run(cuda, a, la, b, lb, w, w)
    alone = _run(cuda, a[2:3], la[2:3], b[2:3], lb[2:3], w[2:3], w[2:3])
    perm = [3, 6, 0, 1, 4, 2, 5]                                                          # pair 2 at position 5, other mates around
    moved = _run(cuda, a[perm], la[perm], b[perm], lb[perm], w[perm], w[perm])
    wide = lambda x: np.concatenate([x, np.full((1, 64 - seq) + x.shape[2:], 7.0, dtype=np.float32)], axis=1)
    padded = _run(cuda, wide(a[2:3]), la[2:3], wide(b[2:3]), lb[2:3], wide(w[2:3]), wide(w[2:3]))
    assert la[2] % 16 and lb[2] % 16
    for name, got in (("alone", alone[0]), ("moved", moved[5]), ("padded to 64", padded[0])):
        assert got.tobytes() == batch[2].tobytes(), (name, got, batch[2])


def test_weight_rules(cuda):
    rng = np.random.default_rng(8)
    hidden, seq_a, seq_b = 64, 40, 21
    la, lb = np.asarray([40, 13, 29, 0, 5], dtype=np.int32), np.asarray([21, 20, 7, 9, 0], dtype=np.int32)
    n = len(la)
    a, b = _states(rng, n, seq_a, seq_b, hidden, np.maximum(la, 1), np.maximum(lb, 1))
    a[0, 3] = 0.0                                            # zero token rows: cosine 0 to everything, never NaN
    b[1, 0] = 0.0
    a[2, :29] = 0.0                                          # a candidate of zero rows only
    none = _run(cuda, a, la, b, lb)
    ones = _run(cuda, a, la, b, lb, np.ones((n, seq_a), np.float32), np.ones((n, seq_b), np.float32))
    assert none.tobytes() == ones.tobytes()                  # NULL = 1 on every real token, bitwise
    assert np.isfinite(none).all()
    assert np.abs(none[:, :2] - bc.match_ref(a, la, b, lb)[:, :2]).max() <= bound(hidden, seq_a, seq_b)
    assert (none[2] == 0).all() and (none[3] == 0).all() and (none[4] == 0).all()       # all-zero side; empty sentences
    wa = np.ones((n, seq_a), np.float32)
    wa[1] = 0.0                                              # a side without weight gives 0 there, and F = 0
    out = _run(cuda, a, la, b, lb, wa, None)
    assert out[1, 0] == 0 and out[1, 2] == 0 and out[1, 1] == none[1, 1] and out[1, 1] != 0
    assert out[0].tobytes() == none[0].tobytes()
    # lens outside [0, seq] are clamped
    big = _run(cuda, a[:1], np.asarray([1000], np.int32), b[:1], np.asarray([-5], np.int32))
    assert (big == 0).all()
    full = _run(cuda, a[:1], np.asarray([1000], np.int32), b[:1], np.asarray([77], np.int32))
    assert full.tobytes() == none[0:1].tobytes()


def test_lane_maps_with_exact_integer_data(cuda):
    """Rows with exactly 16 entries of +-1: every norm is 4, every product, sum and scaling is exact in fp32, so
    sim = dot / 16 exactly.  Pair p weighs candidate token p alone and reference token p % 48 alone: P is row p's maximum and
    R column (p % 48)'s, to the bit.  The expected matrix is not symmetric, within a 16 x 16 tile or across tiles."""
    rng = np.random.default_rng(9)
    hidden, la, lb = 128, 80, 48

    pool = rng.permutation(hidden)[:48]                      # supports drawn from 48 columns spread over both K chunks: dots up to +-16

    def rows(n):
        x = np.zeros((n, hidden), dtype=np.float32)
        for r in range(n):
            x[r, rng.permutation(pool)[:16]] = rng.choice([-1.0, 1.0], 16)
        return x

    a1, b1 = rows(la), rows(lb)
    b1[:12] = a1[rng.permutation(la)[:12]]                   # some exact matches, sim 1
    sim = (a1.astype(np.float64) @ b1.astype(np.float64).T) / 16.0
    assert not np.array_equal(sim[:48, :48], sim[:48, :48].T) and not np.array_equal(sim[:16, :16], sim[:16, :16].T)
    n = la
    a, b = np.broadcast_to(a1, (n, la, hidden)), np.broadcast_to(b1, (n, lb, hidden))
    wa, wb = np.zeros((n, la), np.float32), np.zeros((n, lb), np.float32)
    wa[np.arange(n), np.arange(n)] = 1.0
    wb[np.arange(n), np.arange(n) % lb] = 1.0
    out = _run(cuda, a, np.full(n, la, np.int32), b, np.full(n, lb, np.int32), wa, wb)
    assert np.array_equal(out[:, 0].astype(np.float64), sim.max(1)), np.flatnonzero(out[:, 0] != sim.max(1))
    assert np.array_equal(out[:, 1].astype(np.float64), sim.max(0)[np.arange(n) % lb])
    _check_f(out)
    # unit weights on 64 / 32 tokens: the sums of multiples of 1/16 and the divisions by powers of two are exact, too
    out = _run(cuda, a[:1], np.asarray([64], np.int32), b[:1], np.asarray([32], np.int32))
    s = sim[:64, :32]
    assert out[0, 0] == s.max(1).mean() and out[0, 1] == s.max(0).mean() and s.max(1).mean() != s.max(0).mean()


# ---- end to end against transformers in fp64 ---------------------------------------------------------------------
_scorers = {}


def _scorer(key, layers=None):
    from rag.bertscore import BertScorer
    case = next(c for c in bc.CASES if c[0] == key)
    cfg, seed = case[1], case[2]
    layers = cfg.layers if layers is None else layers
    if (key, layers) not in _scorers:
        _scorers[(key, layers)] = BertScorer({"model_name": key, "num_layers": layers}, shape=bc.model_shape(cfg),
                                             weights=bc.make_weights(cfg, seed), tokenizer=None)
    return _scorers[(key, layers)]


def _golden_scores(key, layers=None):
    import torch
    g = np.load(bc.GOLDEN)
    ma, mb = g[key + ".mask_a"].astype(np.int32), g[key + ".mask_b"].astype(np.int32)
    out = _scorer(key, layers).score_ids_device(g[key + ".ids_a"], ma.sum(1), g[key + ".ids_b"], mb.sum(1))
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64), g[key + ".prf"], g[key + ".prf_prev"], float(g[key + ".min_norm"])


@pytest.mark.parametrize("key", [c[0] for c in bc.CASES])
def test_scorer_matches_the_fp64_golden(cuda, key):
    cfg = next(c for c in bc.CASES if c[0] == key)[1]
    got, want, _prev, min_norm = _golden_scores(key)
    err = np.abs(got - want).max(0)
    print(f"bertscore e2e {key}: max |P| {err[0]:.3e} |R| {err[1]:.3e} |F| {err[2]:.3e}  E2E_TOL {bc.E2E_TOL:.3e}  "
          f"ceiling {bc.e2e_ceiling(cfg.hidden, min_norm):.3e}")
    assert bc.E2E_TOL <= bc.e2e_ceiling(cfg.hidden, min_norm)
    assert err.max() <= bc.E2E_TOL, (key, err)


@pytest.mark.parametrize("key", bc.LAYER_CHECK)
def test_scorer_stops_at_the_requested_layer(cuda, key):
    cfg = next(c for c in bc.CASES if c[0] == key)[1]
    got, at_l, at_prev, _ = _golden_scores(key)
    assert (np.abs(got - at_l).max(1) < np.abs(got - at_prev).max(1)).all()
    got, at_l, at_prev, _ = _golden_scores(key, cfg.layers - 1)
    assert (np.abs(got - at_prev).max(1) < np.abs(got - at_l).max(1)).all()
    assert np.abs(got - at_prev).max() <= bc.E2E_TOL
    assert len(_scorer(key, cfg.layers - 1).model._wlist) == 5 + 12 * (cfg.layers - 1)      # only those layers were uploaded


# ---- the scorer's batching ---------------------------------------------------------------------------------------
WORDS = ("retrieval augmented generation answers questions from compressed documents with a vector index and an encoder on the "
         "device while the metric compares candidate and reference sentences token by token").split()


def _sentences(rng, n):
    out = []
    for _ in range(n):
        k = int(rng.choice([0, 1, 3, 8, 20, 45, 100], p=[0.03, 0.07, 0.2, 0.3, 0.2, 0.1, 0.1]))
        out.append(" ".join(rng.choice(WORDS, k)))
    return out


@pytest.fixture(scope="module")
def tiny_scorer(cuda):
    from rag.bertscore import BertScorer
    return BertScorer({"model_name": "synthetic:tiny", "num_layers": 2, "batch_size": 64})


def test_scorer_batches_ragged_pairs(cuda, tiny_scorer):
    rng = np.random.default_rng(11)
    n = 200
    cands, refs = _sentences(rng, n), _sentences(rng, n)
    cands[0], refs[0] = "", "an empty candidate scores zero"
    cands[1], refs[1] = cands[2], refs[2]                          # duplicates
    cands[3] = " ".join(rng.choice(WORDS, 300))                    # far longer than max_seq_length
    assert max(len(t) for t in tiny_scorer.tokenize(cands)) == tiny_scorer.shape.max_seq == 64
    P, R, F = tiny_scorer.score(cands, refs)
    for x in (P, R, F):
        assert x.shape == (n,) and x.dtype == np.float32 and np.isfinite(x).all()
    assert P[0] == 0 and R[0] == 0 and F[0] == 0
    assert max(abs(P[1] - P[2]), abs(R[1] - R[2]), abs(F[1] - F[2])) <= bc.E2E_TOL      # (they may fall in two batches)
    assert F[4:].max() > 0.3 and F.max() <= 1 + 1e-6
    single = np.stack([np.concatenate(tiny_scorer.score([c], [r])) for c, r in zip(cands, refs)])
    err = np.abs(single - np.stack([P, R, F], 1)).max()
    print(f"bertscore batch vs per-pair: max difference {err:.3e}  E2E_TOL {bc.E2E_TOL:.3e}")
    assert err <= bc.E2E_TOL
    perm = rng.permutation(n)
    P2, R2, F2 = tiny_scorer.score([cands[i] for i in perm], [refs[i] for i in perm])
    assert np.abs(np.stack([P2, R2, F2], 1) - np.stack([P, R, F], 1)[perm]).max() <= bc.E2E_TOL
    empty = tiny_scorer.score([], [])
    assert len(empty) == 3 and all(x.shape == (0,) and x.dtype == np.float32 for x in empty)
    assert tiny_scorer.score_device(cands[:5], refs[:5]).shape == (5, 3)
    with pytest.raises(ValueError, match="one reference per candidate"):
        tiny_scorer.score(cands[:3], refs[:2])


def test_mean_scores_and_the_module_level_score(cuda, tiny_scorer):
    import torch
    from rag import bertscore as bs
    rng = np.random.default_rng(12)
    cands, refs = _sentences(rng, 20), _sentences(rng, 20)
    P, R, F = tiny_scorer.score(cands, refs)
    m = tiny_scorer.mean_scores(cands, refs)
    assert set(m) == {"precision", "recall", "f1"}
    assert m["precision"] == pytest.approx(float(P.mean()), abs=1e-6) and m["recall"] == pytest.approx(float(R.mean()), abs=1e-6)
    assert m["f1"] == pytest.approx(float(F.mean()), abs=1e-6)
    assert tiny_scorer.mean_scores([], []) is None
    out = bs.score(cands, refs, lang="en", verbose=False, model_type="synthetic:tiny", num_layers=2)
    assert len(out) == 3
    for t, want in zip(out, (P, R, F)):
        assert isinstance(t, torch.Tensor) and t.device.type == "cpu" and t.dtype == torch.float32 and t.shape == (20,)
        assert isinstance(t.mean().item(), float)
        assert np.abs(t.numpy() - want).max() <= bc.E2E_TOL
    # idf from the references: rarer tokens weigh more, the scores move but stay scores
    Pi, Ri, Fi = bs.score(cands, refs, model_type="synthetic:tiny", num_layers=2, idf=True)
    assert torch.isfinite(Fi).all() and not torch.equal(Fi, out[2]) and float(Fi.max()) <= 1 + 1e-6
