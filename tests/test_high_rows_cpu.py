"""CPU: the conditions the assertions of tests/test_high_rows_gpu.py rest on (tests/_high_rows.py).

  * the boundary table: every 2^31 / 2^32 byte and element line of every array falls strictly inside [0, N), derived from the
    library's own row lengths, and the planted set holds r - 1, r, r + 1 around each;
  * the alias table: the row a wrapped unsigned offset reaches, for every planted row, array and modulus, lies inside the array and
    carries a score at least MIN_GAP away from the planted row's, for every query -- a kernel that wraps cannot return the
    expected list;
  * the score gaps in fp64;
  * the background generator.

One deviation from a literal "an alias is never a planted row": with lines at 2^19, 2^20, 2^21 and 2^22 and r - 1 planted at each,
row 2^20 - 1 reduced modulo 2^19 rows IS row 2^19 - 1 (and so on up the chain).  Those aliases are planted rows with a DIFFERENT
weight a_i, so their scores differ by at least MIN_GAP for every query; the test asserts exactly that, lists which aliases are
planted, and requires every other alias to be a background row."""
import numpy as np

import _high_rows as hr


def _geometry():
    from rag import _native as nat
    lib = nat.load()
    assert int(lib.crs_padded_dim(hr.DIM)) == int(lib.crs_row_elems(hr.DIM, nat.SLAB_F16))
    return hr.arrays(lib.crs_row_elems(hr.DIM, nat.SLAB_F16), lib.crs_row_elems(hr.DIM, nat.SLAB_I8))


def test_boundary_table():
    geo = _geometry()
    assert hr.N == 2 ** 22 + 1061 and hr.N % 256 == 37 and len(hr.PLANTED_ROWS) == 15 and len(set(hr.PLANTED_ROWS)) == 15
    planted = set(hr.PLANTED_ROWS)
    want = {"shadow": {"2^31 B": 2 ** 19, "2^32 B": 2 ** 20, "2^31 elements": 2 ** 21, "2^32 elements": 2 ** 22},
            "slab f16": {"2^31 B": 2 ** 20, "2^32 B": 2 ** 21, "2^31 elements": 2 ** 21, "2^32 elements": 2 ** 22},
            "slab i8": {"2^31 B": 2 ** 21, "2^32 B": 2 ** 22, "2^31 elements": 2 ** 21, "2^32 elements": 2 ** 22}}
    seen = set()
    for name, (elems, size) in geo.items():
        lines = hr.lines_of(elems, size)
        assert lines == want[name], (name, lines)                   # the derivation gives the lines the module's docstring names
        for mod, r in lines.items():
            assert r is not None and 0 < r - 1 and r + 1 < hr.N, (name, mod, r)
            assert {r - 1, r, r + 1} <= planted, (name, mod, r)
            seen.add(r)
        assert elems * size * hr.N > 2 ** 32 and elems * hr.N > 2 ** 32       # the array really crosses its last line
    assert seen == set(hr.LINES)
    assert {hr.N - 1, 2 ** 22 + 300, 5} <= planted
    assert set(hr.LINE_ROWS) == planted - {2 ** 22 + 300, 5} and len(hr.LINE_ROWS) == 13
    assert hr.VIEW_FIRST == 2 ** 21 + 17


def test_score_gaps_in_fp64():
    q = hr.queries()
    v = hr.planted_vectors()
    assert q.shape == (hr.NQ_MAX, hr.DIM) and not q[:, hr.HEAD:].any()             # the support that makes the 0.2 bound a proof
    assert np.abs(np.sqrt((q.astype(np.float64) ** 2).sum(axis=1)) - 1.0).max() < 1e-6
    assert np.abs(np.sqrt((v.astype(np.float64) ** 2).sum(axis=1)) - 1.0).max() < 1e-6
    s = hr.scores64(q, v)                                                           # [nq, 15]
    assert s.min() >= hr.MIN_PLANTED, s.min()
    srt = -np.sort(-s, axis=1)
    assert (srt[:, :-1] - srt[:, 1:]).min() >= hr.MIN_GAP, (srt[:, :-1] - srt[:, 1:]).min()
    assert hr.MIN_PLANTED - hr.BACKGROUND_MAX > 0.3
    # the weights 0.95 - 0.02 i, each once, and the score order is not the row order
    a = hr.planted_weights()
    assert np.allclose(np.sort(a), np.sort(0.95 - 0.02 * np.arange(15)))
    order = hr.planted_order(q[:1])[0]
    assert sorted(order.tolist()) == sorted(hr.PLANTED_ROWS) and order.tolist() != sorted(order.tolist())
    assert order.tolist() != sorted(order.tolist(), reverse=True)
    # every query ranks the planted rows alike (the score is a_i <q, q0>): one expectation serves all query counts
    assert (hr.planted_order(q) == order[None, :]).all()
    # the near-duplicate join's pairs: every planted pair is clear of the threshold 0.4 by far more than its epsilon (~1.2e-3)
    g = v.astype(np.float64) @ v.astype(np.float64).T
    off = g[~np.eye(15, dtype=bool)]
    assert np.abs(off - 0.4).min() > 0.02, np.abs(off - 0.4).min()


def test_aliases_never_carry_the_planted_score():
    geo = _geometry()
    q = hr.queries()
    s = hr.scores64(q, hr.planted_vectors())                        # [nq, 15]
    col = {r: i for i, r in enumerate(hr.PLANTED_ROWS)}
    planted_aliases, wrapped = set(), 0
    for name, (elems, size) in geo.items():
        for mod_name, m, in_bytes in hr.MODULI:
            for r in hr.PLANTED_ROWS:
                a = hr.alias_row(r, elems, size, m, in_bytes)
                if a is None:
                    assert r * elems * (size if in_bytes else 1) < m
                    continue
                wrapped += 1
                assert 0 <= a < hr.N and a != r, (name, mod_name, r, a)
                if a in col:          # another planted row: a different weight, so a different score for every query
                    planted_aliases.add((r, a))
                    assert np.abs(s[:, col[r]] - s[:, col[a]]).min() >= hr.MIN_GAP, (name, mod_name, r, a)
                # else: a background row, whose score is at most 0.2 < 0.6 - MIN_GAP by Cauchy-Schwarz
    assert wrapped > 60
    # the planted aliases are the chain below each line and nothing else
    assert planted_aliases == {(2 ** 20 - 1, 2 ** 19 - 1), (2 ** 21 - 1, 2 ** 19 - 1), (2 ** 21 - 1, 2 ** 20 - 1), (2 ** 22 - 1, 2 ** 19 - 1),
                               (2 ** 22 - 1, 2 ** 20 - 1), (2 ** 22 - 1, 2 ** 21 - 1)}, sorted(planted_aliases)
    # every planted row but the low-address control wraps in some array; the control never does
    for r in hr.PLANTED_ROWS:
        n_alias = sum(hr.alias_row(r, e, sz, m, b) is not None for e, sz in geo.values() for _, m, b in hr.MODULI)
        assert (n_alias == 0) == (r in (5, 2 ** 19 - 1)), (r, n_alias)
    # the rows a writer test snapshots: inside the array, none of them a written row
    al = hr.alias_rows(hr.LINE_ROWS, geo)
    assert al and all(0 <= a < hr.N for a in al) and not set(al) & set(hr.LINE_ROWS)


def test_compaction_row_maps():
    dead = np.array(sorted({7, 2 ** 20 + 5, 2 ** 21 - 2, 2 ** 22 + 9} | set(range(2 ** 19, 2 ** 19 + 100))))
    keep = np.setdiff1d(np.arange(2 ** 19 + 300), dead)
    for d in (0, 6, 7, 8, 2 ** 19 - 2, 2 ** 19 - 1, 2 ** 19, 2 ** 19 + 150):
        assert hr.source_row(d, dead) == keep[d]
        assert hr.shifted_row(int(keep[d]), dead) == d
    assert hr.source_row(hr.N - len(dead) - 1, dead) == hr.N - 1
    assert hr.source_row(2 ** 22 - 103, dead) == 2 ** 22         # 1 + 100 + 1 + 1 = 103 dead rows lie below 2^22


def test_background_generator():
    import torch
    g = torch.Generator(device="cpu")
    g.manual_seed(hr.SEED)
    x = hr.background(10_000, g, torch.device("cpu"))
    assert x.dtype == torch.float32 and tuple(x.shape) == (10_000, hr.DIM)
    x64 = x.numpy().astype(np.float64)
    assert np.abs(np.sqrt((x64 * x64).sum(axis=1)) - 1.0).max() <= 1e-6
    assert np.abs(np.sqrt((x64[:, :hr.HEAD] ** 2).sum(axis=1)) - hr.HEAD_NORM).max() <= 1e-6
    # hence the bound: |<q, row>| <= |q| x 0.2 for any q supported on the head block
    q = hr.queries(64).astype(np.float64)
    assert np.abs(q @ x64.T).max() <= hr.BACKGROUND_MAX * (1.0 + 1e-5)
    # the int8 image follows csrc/slab_row.h (the model of tests/_slab_ref.py / oracle.scan_ref)
    from oracle import scan_ref
    q8, sc = hr.int8_image(x[:500])
    want_q, want_sc = scan_ref.quantize_rows_i8(x[:500].numpy())
    assert np.array_equal(q8.numpy(), want_q) and np.array_equal(sc.numpy().view(np.uint32), want_sc.view(np.uint32))
