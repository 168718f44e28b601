"""B1 / B3 / B5: ONE encoder layer (and two, for the in-place residual) of TINY, MiniLM and bge-base against the fp64 oracle,
at every token regime that selects different kernels for the same math; the query-batch cases again with
CRS_ENC_SMALL_LDS; the whole file again in child processes under the dispatch's environment switches.

Bound of every comparison: max |gpu - fp64| <= 2 E_q + a (tests/_encoder_cases.py; E_q from the fp16-emulating oracle, a
from the fp32 oracle, both computed per case from the reference alone).  Measured ratios: profiles/enc_cases_ratios.txt.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import _encoder_cases as ec

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ec.LAYER_CASES, ids=lambda c: c.name)
def test_layer_case(cuda, case):
    ec.check_case_on_gpu(case, cuda)


@pytest.mark.parametrize("case", [c for c in ec.LAYER_CASES if c.query_batch], ids=lambda c: c.name)
def test_layer_case_small_lds(cuda, case):
    ec.check_small_lds_on_gpu(case, cuda)


# Kernel forms that production can select by environment and that no default run reaches.  One fresh child per switch (a
# process reads each switch once), one at a time, each under its own timeout; the first failing child ends the test.
SWITCHES = [{"CRS_ATTN_SEQ": "0"}, {"CRS_ATTN_X32": "0"}, {"CRS_ATTN_SHORT": "0"}, {"CRS_ATTN_QT": "4"},
            {"CRS_ROWLN2_VARIANT": "0"}, {"CRS_ENC_BIGLN": "0"}, {"CRS_GEMM8": "0"}]


def test_layer_cases_under_dispatch_switches_in_child_processes(cuda):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for extra in SWITCHES:
        env = dict(os.environ, **extra)
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                            os.path.abspath(__file__), "-k", "test_layer_case and not small_lds and not child"],
                           cwd=root, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, str(extra) + r.stdout[-3000:] + r.stderr[-2000:]
