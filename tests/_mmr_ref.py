"""fp64 restatement of the greedy MMR ordering (ContextRetriever._apply_diversity) and the list generators of the MMR tests.

Everything here is plain numpy in fp64.  A list is (vecs [m, dim], rel [m], lam): position 0 is chosen first; every candidate's
`closest` starts at 0 and becomes max(closest, cos(candidate, newest pick)); value = lam * rel - (1 - lam) * closest; the largest
value wins, equal values go to the lowest position.  A zero vector has cos 0 to everything.

    eps(dim, lam) = 2 (1 - lam) (dim + 8) 2^-24
is the most by which two candidates' values can swap when the cosines are computed in fp32 instead: |fl(a . b) - a . b| <=
dim 2^-24 sum |a_i b_i| <= dim 2^-24 for unit vectors, + 8 units for the two norms (a dot product and a square root each) and
the division, times (1 - lam) for the weight of `closest` in the value, times 2 for the two candidates compared.  It is derived,
not measured."""
import numpy as np


def eps_for(dim, lam):
    return 2.0 * (1.0 - lam) * (dim + 8) * 2.0 ** -24


def cosines(vecs):
    v = np.asarray(vecs, dtype=np.float64)
    g = v @ v.T
    n = np.sqrt(np.diag(g))
    d = np.outer(n, n)
    return np.where(d > 0, g / np.where(d > 0, d, 1.0), 0.0)


def _rounds(cos, rel, lam, pick):
    """Walk the greedy loop; pick(values, pending) chooses each round's position.  Yields (values over pending, pending, chosen)."""
    m = len(rel)
    closest = np.zeros(m)
    pending = list(range(1, m))
    newest = 0
    while pending:
        closest = np.maximum(closest, cos[:, newest])
        values = lam * np.asarray(rel, dtype=np.float64)[pending] - (1.0 - lam) * closest[pending]
        chosen = pick(values, pending)
        yield values, pending, chosen
        pending = [p for p in pending if p != chosen]
        newest = chosen


def mmr_order_ref(vecs, rel, lam):
    """The fp64 order (list of positions); np.argmax returns the first, i.e. lowest, position among equal values."""
    if len(rel) == 0:
        return []
    order = [0]
    for _, _, chosen in _rounds(cosines(vecs), rel, lam, lambda v, p: p[int(np.argmax(v))]):
        order.append(chosen)
    return order


def min_margin(vecs, rel, lam):
    """Smallest gap between the best and the second-best fp64 value over all rounds (inf when no round has two candidates)."""
    gap = np.inf
    if len(rel) == 0:
        return gap
    for values, _, _ in _rounds(cosines(vecs), rel, lam, lambda v, p: p[int(np.argmax(v))]):
        if len(values) > 1:
            top = np.sort(values)[-2:]
            gap = min(gap, float(top[1] - top[0]))
    return gap


def replay_ok(order, vecs, rel, lam, eps):
    """Walk `order` in fp64: every pick's value must be within eps of that round's best.  `order` must be a permutation of
    range(len(rel)) that starts with 0 (the callers assert that first)."""
    order = [int(x) for x in order]
    if len(order) <= 1:
        return True
    it = iter(order[1:])
    for values, pending, chosen in _rounds(cosines(vecs), rel, lam, lambda v, p: next(it)):
        if values[pending.index(chosen)] < values.max() - eps:
            return False
    return True


def store_score(cos):
    """The retriever's score of a hit whose fp32 cosine is `cos`: distance 1 - cos in fp32, then 1 - d^2 / 2 clamped, in fp64."""
    d = (np.float32(1.0) - np.asarray(cos, dtype=np.float32)).astype(np.float64)
    d = np.minimum(np.maximum(d, 0.0), 2.0)
    return np.minimum(np.maximum(1.0 - d * d / 2.0, 0.0), 1.0)


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def ragged_counts(rng, nq, m_max):
    """Counts in [0, m_max], always with 0, 1, 2 and m_max among them."""
    counts = rng.integers(0, m_max + 1, size=nq).astype(np.int32)
    counts[:4] = (0, 1, min(2, m_max), m_max)
    return counts


def make_case(kind, dim, m_max, nq, seed, n_rows=4096):
    """A matrix of n_rows fp32 unit rows, cut into blocks of m_max rows, and nq lists over it.

    kind 'random':  independent gaussian rows; the query of a list is a random unit vector.
    kind 'cluster': per block, max(1, m_max // 4) gaussian centres; a row is a centre plus 0.3 x gaussian noise; the query is the
                    block's row 0 plus 0.5 x a random unit vector.
    List i takes block i % (n_rows // m_max), sorts its rows by fp64 cosine to the query (best first, as a search returns them),
    keeps the first counts[i], and rel is the store's score of each row's cosine."""
    rng = np.random.default_rng(seed)
    nblocks = n_rows // m_max
    vecs = np.zeros((n_rows, dim), dtype=np.float32)
    if kind == "random":
        vecs[:] = _unit(rng.standard_normal((n_rows, dim))).astype(np.float32)
    else:
        for b in range(nblocks):
            centres = rng.standard_normal((max(1, m_max // 4), dim))
            which = rng.integers(0, len(centres), size=m_max)
            vecs[b * m_max:(b + 1) * m_max] = _unit(centres[which] + 0.3 * rng.standard_normal((m_max, dim))).astype(np.float32)
        vecs[nblocks * m_max:] = _unit(rng.standard_normal((n_rows - nblocks * m_max, dim))).astype(np.float32)
    counts = ragged_counts(rng, nq, m_max)
    rows = np.full((nq, m_max), -1, dtype=np.int64)
    rel = np.zeros((nq, m_max), dtype=np.float64)
    for i in range(nq):
        b = i % nblocks
        block = vecs[b * m_max:(b + 1) * m_max].astype(np.float64)
        noise = _unit(rng.standard_normal(dim))
        query = noise if kind == "random" else _unit(block[0] + 0.5 * noise)
        cos = _unit(block) @ query
        best = np.argsort(-cos, kind="stable")[:counts[i]]
        rows[i, :counts[i]] = b * m_max + best
        rel[i, :counts[i]] = store_score(cos[best])
    return {"vecs": vecs, "rows": rows, "rel": rel, "counts": counts}


def list_of(case, i, n_rows=None, base=0):
    """(fp64 vectors, rel) of list i of a case; entries whose row is outside [0, n_rows) are zero vectors."""
    c = int(case["counts"][i])
    rows = case["rows"][i, :c]
    n_rows = case["vecs"].shape[0] - base if n_rows is None else n_rows
    v = np.zeros((c, case["vecs"].shape[1]), dtype=np.float64)
    ok = (rows >= 0) & (rows < n_rows)
    v[ok] = case["vecs"][base + rows[ok]].astype(np.float64)
    return v, case["rel"][i, :c]
