"""On the device: the planner behind crs_scan_plan_describe / crs_scan_workspace_bytes answers what tests/golden/scan_plans.json.xz
recorded before it became a pure function (csrc/plan.cpp), and one search per path through capi.hip's run_scan -- each kernel
family, dump and chain, static and ticketed -- returns the top-k of an fp64 product of the same rows (topk_check.check_topk).

Rows and queries are unit vectors from a seeded numpy generator, rounded to the slab's number format before the reference is
taken (int8: the rows' per-row quantisation and the kernel's 16-bit fixed-point query, oracle/scan_ref.py), so the kernel and
the reference multiply the same numbers.  Each search first asserts the kernel its shape is planned for, so a shape that drifts
into another family fails loudly."""
import functools
import itertools
import json
import lzma
import os

import numpy as np
import pytest

from oracle import scan_ref
from topk_check import check_topk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, I8 = 0, 1
POISON = 0xAB


def test_describe_and_workspace_equal_the_golden_table(cuda):
    """The whole default-knob grid, full text with the cert-tail suffix.  Launches no kernel."""
    import torch
    from rag import _native as nat
    with lzma.open(os.path.join(ROOT, "tests", "golden", "scan_plans.json.xz"), "rt") as f:
        g = json.load(f)
    assert torch.cuda.get_device_properties(cuda).multi_processor_count == g["cus"], "the table was recorded for another CU count"
    s = g["settings"][0]
    assert s["env"] == {} and g["order"] == ["slab_type", "dim", "nq", "k", "n_rows"]
    grid = g["grid"]
    half = len(s["bytes"])
    bad = []
    for i, (st, dim, nq, k, n) in enumerate(itertools.product(grid["slab_type"], grid["dim"], grid["nq"], grid["k"], grid["n_rows"])):
        text = nat.scan_plan_describe(nq, dim, k, n, slab_type=st)
        if text != g["texts"][s["text"][i]]:
            bad.append(((nq, dim, k, n, st), text, g["texts"][s["text"][i]]))
        if st == F16 and nat.scan_workspace_bytes(nq, dim, k, n) != g["sizes"][s["bytes"][i % half]]:
            bad.append(((nq, dim, k, n), nat.scan_workspace_bytes(nq, dim, k, n), g["sizes"][s["bytes"][i % half]]))
    assert not bad, "%d cases differ, first: %s" % (len(bad), bad[:3])


def _unit(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d), dtype=np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _slab(n, d, st):
    """(the rows as they go to the device, per-row scales or None)"""
    rows = _unit(n, d, 100 + d)
    if st == I8:
        c8, sc = scan_ref.quantize_rows_i8(rows)
        return c8, sc
    return rows.astype(np.float16), None


@functools.lru_cache(maxsize=None)
def _queries(d):
    return _unit(256, d, 200 + d).astype(np.float16)


@functools.lru_cache(maxsize=None)
def _full64(n, d, st, nq):
    """fp64 scores of the first nq queries against every row, in blocks of rows (computed once per slab and query count)"""
    slab, scales = _slab(n, d, st)
    q = _queries(d)[:nq]
    q64 = scan_ref.dequantized_queries(q) if st == I8 else q.astype(np.float64)
    out = np.empty((nq, n), dtype=np.float64)
    for lo in range(0, n, 32768):
        out[:, lo:lo + 32768] = q64 @ slab[lo:lo + 32768].astype(np.float64).T
    if scales is not None:
        out *= scales.astype(np.float64)[None, :]
    out.setflags(write=False)
    return out


# (path through run_scan, rows, row length, slab type, queries, k, knobs set inside the process, kernel in the describe text,
#  whether the launch draws tiles from the ticket: True / False, None where the form has none)
PATHS = [
    ("tile-best dump", 4096, 384, F16, 64, 10, {}, "scan_tb_kernel<384,32,4,0>", None),
    ("tile-best chain, static", 300_000, 128, F16, 64, 16, {}, "scan_tb_kernel<128,32,4,16>", False),
    ("tile-best chain, ticketed", 300_000, 128, F16, 64, 16, {"CRS_TB_DYN_MIN": "4"}, "scan_tb_kernel<128,32,4,16>", True),
    ("long chain", 300_000, 128, F16, 64, 24, {}, "scan_tb_kernel<128,32,4,24>", False),
    ("classic through the fall-through", 300_000, 512, F16, 64, 64, {}, "scan_f16_kernel<512,32,32>", None),
    ("wide, 4 waves", 20_000, 384, F16, 128, 16, {}, "scan_wide_kernel<384,4,16>", None),
    ("wide, 8 waves", 20_000, 384, F16, 256, 16, {}, "scan_wide_kernel<384,8,16>", None),
    ("wide, 8 waves, streamed, 16x16x32", 20_000, 384, F16, 256, 24, {}, "scan_wide_kernel<384,8,24>", False),
    ("w1", 20_000, 768, F16, 256, 16, {}, "scan_w2_kernel<768>", None),
    ("int8 dump", 4096, 768, I8, 64, 10, {}, "scan_i8_kernel<768,32,16,0>", None),
    ("int8 chain", 300_000, 768, I8, 64, 10, {}, "scan_i8_kernel<768,32,16,10>", False),
]


@pytest.mark.parametrize("path,n,d,st,nq,k,env,kernel,ticket", PATHS, ids=[p[0] for p in PATHS])
def test_one_search_per_path_through_run_scan(cuda, path, n, d, st, nq, k, env, kernel, ticket):
    import torch
    from rag import _native as nat
    slab_np, scales_np = _slab(n, d, st)
    assert nat.padded_dim(d, st) == d
    slab = torch.from_numpy(slab_np).to(cuda)
    scales = torch.from_numpy(scales_np).to(cuda) if st == I8 else None
    q = torch.from_numpy(_queries(d)[:nq]).to(cuda)
    old = {name: os.environ.get(name) for name in env}
    os.environ.update(env)
    try:
        text = nat.scan_plan_describe(nq, d, k, n, slab_type=st)
        assert text.startswith(kernel), (path, text)
        ws = torch.full((nat.scan_workspace_bytes(nq, d, k, n),), POISON, dtype=torch.uint8, device=cuda)
        sc, ids = nat.cosine_topk(q, slab, n, d, k, slab_type=st, scales=scales, workspace=ws)
        torch.cuda.synchronize()
    finally:
        for name, v in old.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v
    word = int(ws[:4].view(torch.int32)[0])
    if ticket is True:      # the counter at the head of the workspace was zeroed and drawn from
        assert 0 < word < n, (path, word)
    elif ticket is False:   # a static launch leaves the workspace's first word alone
        assert word == int(np.array([POISON] * 4, dtype=np.uint8).view(np.int32)[0]), (path, word)
    check_topk(sc.cpu().numpy(), ids.cpu().numpy(), _full64(n, d, st, nq), k)
