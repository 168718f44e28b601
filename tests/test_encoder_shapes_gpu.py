"""B2 / B3: the model space crs_encoder's check_desc accepts (hidden % 64 == 0 up to 1024, head_dim 16 / 32 / 64,
ffn % 64 == 0) and the token counts on both sides of every dispatch threshold, 1-2 layers each, against the fp64 oracle
with the bound 2 E_q + a of tests/_encoder_cases.py.  Every forward runs in a workspace of exactly
crs_encoder_workspace_bytes with a poisoned guard region behind it.  The kernels each case launched on an MI355X are listed
in profiles/enc_cases_kernels.txt (tools/enc_case_kernels.py), the measured ratios in profiles/enc_cases_ratios.txt.
"""
import ctypes

import numpy as np
import pytest

import _encoder_cases as ec

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ec.SHAPE_CASES, ids=lambda c: c.name)
def test_shape_case(cuda, case):
    ec.check_case_on_gpu(case, cuda)


@pytest.mark.parametrize("case", [c for c in ec.SHAPE_CASES if c.query_batch], ids=lambda c: c.name)
def test_shape_case_small_lds(cuda, case):
    ec.check_small_lds_on_gpu(case, cuda)


@pytest.mark.parametrize("hidden,heads,ffn", [(96, 3, 256), (1088, 17, 4096), (384, 3, 1536), (384, 48, 1536), (384, 12, 1000), (384, 5, 1536)])
def test_descriptors_outside_the_space_are_refused_before_any_launch(cuda, hidden, heads, ffn):
    from rag import _native as nat
    from rag._encoder import EncoderDesc
    d = EncoderDesc(1000, hidden, 1, heads, ffn, 64, 1e-12, 0, 0)
    out = ctypes.c_size_t(0)
    assert nat.load().crs_encoder_workspace_bytes(ctypes.byref(d), 2, 16, ctypes.byref(out)) == -1     # CRS_EINVAL
    assert out.value == 0
