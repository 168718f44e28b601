"""CPU restatement (numpy) of the inner-product / squared-L2 transform of csrc/space.hip, for the space tests.

A store of space 'ip' / 'l2' keeps one scale R = 2^e >= every row norm and stores
    ip:  u = x / R                                  query  q / |q|
    l2:  (v, t), v = x / (2R), t = fl32(sum v_i^2)   query  (q / R, -1) / |(q / R, -1)|
so that the cosine scan's descending score is the space's ascending distance.  Everything here is fp32 where the device is
fp32 (the scaling, t) and fp64 where a test needs a reference (the metrics, the rankings, the bounds).  t is summed in ONE fixed
order (left to right in fp32); the device uses another fixed order, so t is compared between stores built by the same code,
never across the two.
"""
import numpy as np

SPACES = ("ip", "l2")
U = 2.0 ** -24          # fp32 unit roundoff


def norm_scale_for(norm_max: float) -> float:
    """The smallest power of two >= norm_max (1.0 for 0)."""
    if not norm_max > 0.0:
        return 1.0
    m, e = np.frexp(np.float64(norm_max))
    return float(np.ldexp(1.0, int(e) - 1 if m == 0.5 else int(e)))


def row_norm_max(x32: np.ndarray) -> float:
    return float(np.sqrt((x32.astype(np.float64) ** 2).sum(axis=1)).max()) if len(x32) else 0.0


def _t_of(v32: np.ndarray) -> np.ndarray:
    """fl32(sum v_i^2), left to right, every operation rounded to fp32."""
    t = np.zeros(v32.shape[0], dtype=np.float32)
    for c in range(v32.shape[1]):
        t = (t + v32[:, c] * v32[:, c]).astype(np.float32)
    return t


def store_rows(x32: np.ndarray, space: str, R: float) -> np.ndarray:
    """The fp32 rows a store of scale R keeps for the vectors x32 [n, d]: [n, d] (ip) or [n, d + 1] (l2)."""
    x32 = np.asarray(x32, dtype=np.float32)
    if space == "ip":
        return (x32 * np.float32(1.0 / R)).astype(np.float32)
    v = (x32 * np.float32(0.5 / R)).astype(np.float32)
    return np.concatenate([v, _t_of(v)[:, None]], axis=1)


def rescale_rows(rows32: np.ndarray, space: str, shift: int) -> np.ndarray:
    """What the stored rows become when R grows to R 2^shift: every coordinate times 2^-shift, l2's last times 2^-2 shift."""
    out = (rows32 * np.float32(2.0 ** -shift)).astype(np.float32)
    if space == "l2":
        out[:, -1] = rows32[:, -1] * np.float32(2.0 ** (-2 * shift))
    return out


def recover(rows32: np.ndarray, space: str, R: float) -> np.ndarray:
    """The caller's vectors back from the stored rows: x = R u (ip), x = 2R v (l2)."""
    if space == "ip":
        return (rows32 * np.float32(R)).astype(np.float32)
    return (rows32[:, :-1] * np.float32(2.0 * R)).astype(np.float32)


def queries(q32: np.ndarray, space: str, R: float) -> np.ndarray:
    """The unit queries the scan sees, in fp64."""
    q = np.asarray(q32, dtype=np.float64)
    if space == "l2":
        q = np.concatenate([q / R, -np.ones((q.shape[0], 1))], axis=1)
    return q / np.maximum(np.sqrt((q * q).sum(axis=1, keepdims=True)), 1e-12)


def metric64(q32: np.ndarray, x32: np.ndarray, space: str) -> np.ndarray:
    """ChromaDB's distance in fp64, [nq, n]: 1 - <q, x> (ip), sum (q - x)^2 (l2).  Ascending = better."""
    q, x = np.asarray(q32, dtype=np.float64), np.asarray(x32, dtype=np.float64)
    if space == "ip":
        return 1.0 - q @ x.T
    return ((q * q).sum(axis=1)[:, None] - 2.0 * (q @ x.T)) + (x * x).sum(axis=1)[None, :]


def metric64_rows(q32_row: np.ndarray, x32: np.ndarray, space: str) -> np.ndarray:
    """The same for one query against a few rows, summed directly (no expansion of the square): the distances' reference."""
    q, x = np.asarray(q32_row, dtype=np.float64), np.asarray(x32, dtype=np.float64)
    if space == "ip":
        return 1.0 - (x * q[None, :]).sum(axis=1)
    return ((q[None, :] - x) ** 2).sum(axis=1)


def distance_tol(q32_row: np.ndarray, x32: np.ndarray, space: str) -> np.ndarray:
    """(d + 2) 2^-24 sum |q_i x_i| (ip) or (d + 2) 2^-24 sum (q_i - x_i)^2 (l2), per row: the bound on a distance."""
    q, x = np.asarray(q32_row, dtype=np.float64), np.asarray(x32, dtype=np.float64)
    mass = np.abs(x * q[None, :]).sum(axis=1) if space == "ip" else ((q[None, :] - x) ** 2).sum(axis=1)
    return (x.shape[1] + 2) * U * mass


def swap_tol(q32: np.ndarray, d: int, space: str, R: float) -> np.ndarray:
    """Per query, the fp64 metric gap below which two rows may change places: the fp32 ranking of the transformed rows differs
    from the true one by at most the rounding of a d'-term fp32 dot product of unit-bounded vectors, 2 (d' + 4) 2^-24, mapped back
    to the metric's units -- |q| R per unit of score (ip), 4 R^2 |(q / R, -1)| (l2)."""
    q = np.asarray(q32, dtype=np.float64)
    qn = np.sqrt((q * q).sum(axis=1))
    if space == "ip":
        return 2 * (d + 4) * U * qn * R
    return 2 * (d + 1 + 4) * U * 4 * R * R * np.sqrt(qn * qn / (R * R) + 1.0)


def ranking(metric_row: np.ndarray) -> np.ndarray:
    """Rows by (metric asc, row asc)."""
    return np.lexsort((np.arange(metric_row.shape[0]), metric_row))


def topk_errors(got_i: np.ndarray, metric: np.ndarray, k: int, tol: np.ndarray) -> dict:
    """The near-tie rule of tests/topk_check.py::topk_errors on a metric where smaller is better: {query: reason} for every
    list that is not the fp64 ranking's first k rows up to swaps between rows whose fp64 metric values differ by less than
    tol[query]; every returned row must also lie within tol of the k-th best."""
    errs = {}
    for r in range(got_i.shape[0]):
        ref = ranking(metric[r])[:k]
        got = got_i[r, :k]
        if (got < 0).any() or len(set(got.tolist())) != k:
            errs[r] = f"got rows {got.tolist()}"
            continue
        kth = metric[r, ref[k - 1]]
        for a, b in zip(got.tolist(), ref.tolist()):
            if a != b and not abs(metric[r, a] - metric[r, b]) < tol[r]:
                errs[r] = f"got row {a} ({metric[r, a]!r}), reference row {b} ({metric[r, b]!r}), tol {tol[r]!r}"
                break
        else:
            if not (metric[r, got] <= kth + tol[r]).all():
                errs[r] = "a row beyond the k-th best was returned"
    return errs


def kth_gaps(metric: np.ndarray, ks) -> np.ndarray:
    """[nq, len(ks)]: the fp64 gap between the k-th and the (k + 1)-th best row of every query."""
    srt = np.sort(metric, axis=1)
    return np.stack([srt[:, k] - srt[:, k - 1] for k in ks], axis=1)


def make_rows(n: int, d: int, seed: int, lo: float = 0.24, hi: float = 1.95) -> np.ndarray:
    """n random fp32 rows whose norms are spread over [lo, hi] (8 x and more); the two extremes are planted, so
    R = norm_scale_for(hi) = 2 for the defaults."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d))
    x /= np.sqrt((x * x).sum(axis=1, keepdims=True))
    # squared norms thin out towards the short end (density ~ (s - lo^2)^2): under l2 the nearest rows of a query are the short
    # ones, and a log-uniform spread would put their distances closer together than any fp32 ranking can tell apart (swap_tol)
    norms = np.sqrt(lo * lo + (hi * hi - lo * lo) * rng.uniform(size=n) ** (1.0 / 3.0))
    norms[0], norms[1] = lo, hi
    return (x * norms[:, None]).astype(np.float32)


def pick_queries(x32: np.ndarray, space: str, R: float, nq: int, ks, seed: int, pool: int = 4096) -> np.ndarray:
    """nq fp32 queries (norms around 1) chosen from a seeded pool so that, for each, the fp64 gap at every k of `ks` exceeds twice
    swap_tol: the inputs are chosen so that the tolerance cannot be what makes a test pass.  The caller asserts the gaps again."""
    rng = np.random.default_rng(seed)
    d = x32.shape[1]
    q = rng.standard_normal((pool, d))
    q *= (rng.uniform(0.7, 1.4, size=(pool, 1)) / np.sqrt((q * q).sum(axis=1, keepdims=True)))
    q = q.astype(np.float32)
    ok = (kth_gaps(metric64(q, x32, space), [k for k in ks if k < len(x32)]) > 2.0 * swap_tol(q, d, space, R)[:, None]).all(axis=1)
    keep = np.flatnonzero(ok)[:nq]
    assert len(keep) == nq, f"only {len(keep)} of {pool} candidate queries have clear gaps at {ks}"
    return q[keep]
