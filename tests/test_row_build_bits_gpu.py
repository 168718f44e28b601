"""GPU: the row writers (slab_store_row, csrc/slab_row.h, through csrc/row_build.hip) against the recorded bits of
tests/golden/row_build_bits.npz -- slab, int8 scales, fp32 shadow and row error of the cosine, ip and l2 appends and of
crs_queries_to_f16, byte for byte.  tests/_row_bits.py lists the cases and says why the bits are pinned; tools/ab_row_build.py
recorded the fixture (its `record` mode).  Scatter and rescale are tied to the append bit for bit by test_mutate_gpu.py and
test_space_build_gpu.py.
"""
import os

import numpy as np
import pytest

import _row_bits as rb

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_build_bits.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_fixture_holds_every_case(golden):
    want = {rb.input_key(kind, dim, R) for kind, st, dim, R in rb.CASES}
    for kind, st, dim, R in rb.CASES:
        names = ("slab",) if kind == "q16" else tuple(a for a in rb.ARRAYS if a != "scales" or st == rb.I8)
        want |= {rb.key(kind, st, dim, R) + "/" + a for a in names}
    assert set(golden) == want
    assert os.path.getsize(GOLDEN) < 512 * 1024


@pytest.mark.parametrize("kind,st,dim,R", rb.CASES, ids=[rb.key(*c) for c in rb.CASES])
def test_rows_equal_the_recorded_bits(cuda, golden, kind, st, dim, R):
    x = golden[rb.input_key(kind, dim, R)]
    assert x.dtype == np.float32 and x.shape == (rb.N_ROWS, dim)
    got = rb.run_case(kind, st, dim, R, x, cuda)
    for name, arr in got.items():
        want = golden[rb.key(kind, st, dim, R) + "/" + name]
        assert arr.dtype == want.dtype and arr.shape == want.shape, name
        diff = np.count_nonzero(np.ascontiguousarray(arr).view(np.uint8) != np.ascontiguousarray(want).view(np.uint8))
        assert diff == 0, f"{name}: {diff} bytes differ from the recorded row"
