"""Geometry, data and fp64 expectations of the high-row tests (tests/test_high_rows_cpu.py, tests/test_high_rows_gpu.py).

Every kernel that takes a row number forms an address as row * row_elems.  The store built here is large enough that this product
leaves 32 bits inside every array, and it is built so that a kernel which wraps it returns a visibly different answer:

  * cosine space, dim 1024 (the widest row: the fewest rows reach each line), N = 2^22 + 1061 rows (1061 = 4 x 256 + 37, ragged
    against every tile size);
  * background rows [0.2 h, sqrt(0.96) t], h a random unit vector on coordinates [0, 64), t one on [64, 1024);
  * queries supported on [0, 64): <q, background row> = 0.2 <q, h> <= 0.2 by Cauchy-Schwarz, whatever the arithmetic;
  * 15 planted rows a_i q0 + sqrt(1 - a_i^2) u_i (u_i a unit vector on [64, 1024), so <q, planted_i> = a_i <q, q0>) on both sides of
    every line, the a_i assigned in shuffled order so that score order is not row order.

A wrapped offset inside such an array lands on another row of the same array: no fault, no NaN.  The alias table below names that
row for every planted row, array and wrap modulus; the CPU test shows that it never carries the planted row's score.

Plain numpy here; torch only inside the functions that take a device.  The padded row lengths come from the library (the caller
passes them in), never from constants of this file.
"""
from __future__ import annotations

import numpy as np

DIM = 1024
HEAD = 64                                   # the queries' support, and the background rows' head block
N = (1 << 22) + 1061
CHUNK = 262_144                             # rows written at a time
LINES = (1 << 19, 1 << 20, 1 << 21, 1 << 22)
LINE_ROWS = tuple(x + o for x in LINES for o in (-1, 0, 1)) + (N - 1,)        # the 13 rows a scatter writes
PLANTED_ROWS = tuple(sorted(LINE_ROWS + ((1 << 22) + 300, 5)))                # + one more high row and a low-address control
N_PLANTED = len(PLANTED_ROWS)
HEAD_NORM = 0.2
BACKGROUND_MAX = 0.2                        # the proof's bound on every background score
MIN_PLANTED = 0.6
MIN_GAP = 0.015
MODULI = (("2^31 B", 1 << 31, True), ("2^32 B", 1 << 32, True), ("2^31 elements", 1 << 31, False), ("2^32 elements", 1 << 32, False))
SEED = 20_261_020
VIEW_FIRST = (1 << 21) + 17                 # the second run of the scan: slab[VIEW_FIRST:], id_base = VIEW_FIRST
NQ_MAX = 256


# ------------------------------------------------------------------------------------------------------------------ geometry
def arrays(row_elems_f16: int, row_elems_i8: int) -> dict:
    """name -> (elements per row, bytes per element).  The row lengths are crs_row_elems(DIM, slab_type) of the library."""
    return {"shadow": (DIM, 4), "slab f16": (int(row_elems_f16), 2), "slab i8": (int(row_elems_i8), 1)}


def lines_of(row_elems: int, elem_bytes: int) -> dict:
    """modulus name -> the first row whose offset reaches the modulus (None: a row straddles it, or no row reaches it)."""
    out = {}
    for name, m, in_bytes in MODULI:
        per_row = row_elems * (elem_bytes if in_bytes else 1)
        out[name] = m // per_row if m % per_row == 0 else None
    return out


def alias_row(row: int, row_elems: int, elem_bytes: int, modulus: int, in_bytes: bool):
    """The row a kernel reaches when row * row_elems (x the element size when the offset is formed in bytes) is reduced modulo
    `modulus` as an unsigned offset; None when the offset does not wrap (the kernel reaches the right row)."""
    per_row = row_elems * (elem_bytes if in_bytes else 1)
    off = row * per_row
    if off < modulus:
        return None
    assert modulus % per_row == 0
    return (off % modulus) // per_row


def alias_rows(rows, geometry: dict, names=None) -> list:
    """Every alias of `rows` in the named arrays (all of them by default), without the rows themselves: what a writer test
    snapshots beside the rows it writes."""
    rows = [int(r) for r in rows]
    out = set()
    for name, (elems, size) in geometry.items():
        if names is not None and name not in names:
            continue
        for _, m, in_bytes in MODULI:
            for r in rows:
                a = alias_row(r, elems, size, m, in_bytes)
                if a is not None:
                    out.add(a)
    return sorted(out - set(rows))


def source_row(d: int, dead_sorted) -> int:
    """The row that a stable compaction without the rows `dead_sorted` moves to row d."""
    dead = np.asarray(dead_sorted)
    s = int(d)
    while True:
        s2 = int(d) + int(np.searchsorted(dead, s, side="right"))
        if s2 == s:
            return s
        s = s2


def shifted_row(s: int, dead_sorted) -> int:
    """Where a surviving row s sits after that compaction."""
    return int(s) - int(np.searchsorted(np.asarray(dead_sorted), s, side="left"))


# ------------------------------------------------------------------------------------------------------------------ host data
def _unit(x):
    return x / np.sqrt((x * x).sum(axis=-1, keepdims=True))


def base_query() -> np.ndarray:
    """q0: a unit vector on coordinates [0, HEAD), float64 [DIM]."""
    rng = np.random.default_rng(SEED)
    q0 = np.zeros(DIM)
    q0[:HEAD] = _unit(rng.standard_normal(HEAD))
    return q0


def queries(nq: int = NQ_MAX) -> np.ndarray:
    """q_j = normalize(q0 + 0.25 g_j), g_j unit on [0, HEAD): fp32 [nq, DIM]; the first nq of one fixed sequence."""
    rng = np.random.default_rng(SEED + 1)
    g = np.zeros((NQ_MAX, DIM))
    g[:, :HEAD] = _unit(rng.standard_normal((NQ_MAX, HEAD)))
    return np.ascontiguousarray(_unit(base_query()[None, :] + 0.25 * g).astype(np.float32)[:nq])


def planted_weights() -> np.ndarray:
    """a_i of PLANTED_ROWS[i]: the values 0.95 - 0.02 j in shuffled order."""
    rng = np.random.default_rng(SEED + 2)
    return (0.95 - 0.02 * np.arange(N_PLANTED))[rng.permutation(N_PLANTED)]


def planted_vectors() -> np.ndarray:
    """fp32 [N_PLANTED, DIM], row i for store row PLANTED_ROWS[i]."""
    rng = np.random.default_rng(SEED + 3)
    a = planted_weights()[:, None]
    u = np.zeros((N_PLANTED, DIM))
    u[:, HEAD:] = _unit(rng.standard_normal((N_PLANTED, DIM - HEAD)))
    return np.ascontiguousarray((a * base_query()[None, :] + np.sqrt(1.0 - a * a) * u).astype(np.float32))


def scores64(q, rows) -> np.ndarray:
    """[nq, n] = <q_j, row_i> in float64."""
    return np.asarray(q).astype(np.float64) @ np.asarray(rows).astype(np.float64).T


def order64(scores_row, ids) -> np.ndarray:
    """ids by (score desc, id asc)."""
    ids = np.asarray(ids)
    return ids[np.lexsort((ids, -np.asarray(scores_row, dtype=np.float64)))]


def planted_order(q, planted_rows32=None, rows=PLANTED_ROWS) -> np.ndarray:
    """int64 [nq, len(rows)]: the planted store rows in the fp64 order of their scores, per query.  planted_rows32: the fp32 rows
    as the store holds them (host copies), planted_vectors() by default."""
    v = planted_vectors() if planted_rows32 is None else planted_rows32
    s = scores64(q, v)
    return np.stack([order64(s[j], np.asarray(rows, dtype=np.int64)) for j in range(s.shape[0])])


# ------------------------------------------------------------------------------------------------------------------ the store
def background(m: int, generator, device):
    """m background rows, fp32 [m, DIM] on `device`: [0.2 h, sqrt(0.96) t] with h, t random unit vectors.  Plain torch."""
    import torch
    x = torch.randn((m, DIM), generator=generator, device=device, dtype=torch.float32)
    head, tail = x[:, :HEAD], x[:, HEAD:]
    head *= HEAD_NORM / head.norm(dim=1, keepdim=True)
    tail *= float(np.sqrt(1.0 - HEAD_NORM * HEAD_NORM)) / tail.norm(dim=1, keepdim=True)
    return x


def int8_image(x):
    """(int8 rows, fp32 scales) of fp32 rows by the rule of csrc/slab_row.h (tests/_slab_ref.py models the same): scale =
    max|x| / 127, q = rint(x / scale) clamped to +-127.  Plain torch."""
    import torch
    sc = x.abs().amax(dim=1) / 127.0
    safe = torch.where(sc > 0, sc, torch.ones_like(sc))
    q = torch.round(x / safe[:, None]).clamp_(-127.0, 127.0).to(torch.int8)
    return q, sc


class Store:
    """The three arrays of the store on one device, written with plain torch: shadow fp32 [N, DIM], slab fp16 [N, pdim16],
    slab8 int8 [N, pdim8] + scales fp32 [N].  rebuild() regenerates all of it from the seed."""

    def __init__(self, device, pdim16: int, pdim8: int):
        import torch
        assert pdim16 == DIM and pdim8 == DIM, "dim 1024 needs no padding in either slab"
        self.device = device
        self.shadow = torch.empty((N, DIM), dtype=torch.float32, device=device)
        self.slab = torch.empty((N, pdim16), dtype=torch.float16, device=device)
        self.slab8 = torch.empty((N, pdim8), dtype=torch.int8, device=device)
        self.scales = torch.empty(N, dtype=torch.float32, device=device)
        self.planted = torch.tensor(PLANTED_ROWS, dtype=torch.int64, device=device)
        self.rebuild()

    def rebuild(self):
        import torch
        g = torch.Generator(device=self.device)
        g.manual_seed(SEED)
        for lo in range(0, N, CHUNK):
            hi = min(N, lo + CHUNK)
            x = background(hi - lo, g, self.device)
            self.put(slice(lo, hi), x)
            del x
        self.put(self.planted, torch.from_numpy(planted_vectors()).to(self.device))
        torch.cuda.synchronize(self.device)

    def put(self, where, x):
        """rows `where` (a slice or an index tensor) of all three arrays <- the fp32 rows x."""
        self.shadow[where] = x
        self.slab[where] = x.half()
        q, sc = int8_image(x)
        self.slab8[where] = q
        self.scales[where] = sc

    def arrays_of(self, slab_type: int):
        """(slab, scales or None) of a slab type (0 fp16, 1 int8)."""
        return (self.slab8, self.scales) if slab_type else (self.slab, None)

    def free(self):
        self.shadow = self.slab = self.slab8 = self.scales = self.planted = None
