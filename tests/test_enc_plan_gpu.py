"""On the device: crs_encoder_plan_describe and crs_encoder_workspace_bytes answer what tests/golden/enc_plans.json.xz recorded from a
kernel trace before the encoder's planner existed (csrc/enc_plan.cpp; the same file tests/test_enc_plan_cpu.py holds the planner to
on a CPU), a forward captured into a graph -- the plan is made inside the capture -- replays the bits of the eager forward, and a
describe buffer that is too small is respected.  The kernels and their launches are the per-case suites' business
(test_encoder_layer_gpu.py, test_encoder_shapes_gpu.py, test_encoder_hard_gpu.py)."""
import ctypes
import json
import lzma
import os
import re
import sys

import numpy as np
import pytest

import _encoder_cases as ec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))      # enc_case_kernels.py: the models of the byte table


@pytest.fixture(scope="module")
def golden():
    with lzma.open(os.path.join(ROOT, "tests", "golden", "enc_plans.json.xz"), "rt") as f:
        g = json.load(f)
    assert g["settings"][0]["env"] == {}
    return g


def desc_of(hidden, heads, ffn, layers, max_pos, flags=0):
    from rag._encoder import EncoderDesc
    return EncoderDesc(1000, hidden, layers, heads, ffn, max_pos, 1e-12, 0, flags)


def test_workspace_bytes_equal_the_golden(cuda, golden):
    """every multiple of 16 tokens up to 8192 and the larger counts, nine models; the byte counts depend on no CU count"""
    from rag import _native as nat
    import enc_case_kernels as eck
    lib = nat.load()
    out = ctypes.c_size_t(0)
    bad = []
    for name, cfg in eck.grid_models():
        d = desc_of(cfg.hidden, cfg.heads, cfg.ffn, cfg.layers, cfg.max_pos)
        for t, i in zip(golden["bytes_tokens"], golden["settings"][0]["bytes"][name]):
            nat.check(lib.crs_encoder_workspace_bytes(ctypes.byref(d), t // 16, 16, ctypes.byref(out)))
            if out.value != golden["sizes"][i]:
                bad.append((name, t, out.value, golden["sizes"][i]))
    assert not bad, "%d byte counts differ, first: %s" % (len(bad), bad[:3])


def test_describe_equals_the_golden_launches(cuda, golden):
    """every forward of the default setting: the cases (default and small-LDS), relative bias, pair head, both grids.  Launches no kernel."""
    import torch
    from rag import _native as nat
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    if cus != golden["cus"]:
        pytest.skip(f"this device has {cus} CUs, the launch record was made on {golden['cus']}: grids and forms differ (the byte counts are compared)")
    no_lds = lambda line: re.sub(r" lds=\d+$", "", line)
    bad = []
    for c in golden["settings"][0]["calls"]:
        if c["kind"] != "fwd":
            continue
        text = nat.encoder_plan_describe(desc_of(c["hidden"], c["heads"], c["ffn"], c["layers"], c["max_pos"], c["small"]), c["batch"], c["seq"],
                                         rel_bias=bool(c["rel"]), pair=c["pair"]).splitlines()
        got = [no_lds(t) for t in text[:1] + text[1:-1] * c["layers"] + text[-1:]]
        want = [no_lds(golden["texts"][i]) for i in golden["lists"][c["list"]]]
        if got != want:
            bad.append((c["name"], c["small"], got, want))
    assert not bad, "%d forwards differ, first: %s" % (len(bad), bad[:2])


@pytest.mark.parametrize("name", ["minilm-8x16", "bge-8x16"])
def test_graph_replay_gives_the_bits_of_the_eager_forward(cuda, name):
    import torch
    case = next(c for c in ec.ALL_CASES if c.name == name)
    enc = ec.hip_encoder(case, cuda)
    ids, _, lens = ec.case_inputs(case)
    ids_d, lens_d = torch.from_numpy(ids).to(cuda), torch.from_numpy(lens).to(cuda)
    ws = torch.empty(enc.workspace_bytes(case.batch, case.seq), dtype=torch.uint8, device=cuda)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        want, want_h = enc.forward(ids_d, lens_d, return_hidden=True, workspace=ws)
        want, want_h = want.clone(), want_h.clone()
    torch.cuda.current_stream().wait_stream(st)
    out = torch.empty_like(want)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, hidden = enc.forward(ids_d, lens_d, return_hidden=True, out=out, workspace=ws)
    for _ in range(2):
        out.fill_(float("nan"))
        hidden.fill_(float("nan"))
        ws.fill_(0xA5)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want) and torch.equal(hidden, want_h)
    assert np.isfinite(want.cpu().numpy()).all()


def test_describe_respects_a_small_buffer(cuda):
    """returns the length of the whole text and writes no byte past cap (the cut text is terminated inside it)"""
    from rag import _native as nat
    lib = nat.load()
    d = desc_of(384, 12, 1536, 1, 512)
    full = nat.encoder_plan_describe(d, 8, 16)
    assert full.count("\n") == 8 and full.startswith("embed_ln2_kernel<3, false> grid=32x1x1 wg=256x1x1 lds=0\n")
    for cap in (0, 1, 17, len(full), len(full) + 1):
        buf = ctypes.create_string_buffer(b"\xa5" * 4096, 4096)
        assert lib.crs_encoder_plan_describe(ctypes.byref(d), 8, 16, 0, 0, buf, cap) == len(full)
        raw = buf.raw
        assert raw[cap:] == b"\xa5" * (4096 - cap), cap
        if cap:
            n = min(cap - 1, len(full))
            assert raw[:n] == full.encode()[:n] and raw[n] == 0, cap
    assert lib.crs_encoder_plan_describe(ctypes.byref(d), 8, 16, 0, 0, None, 0) == len(full)
    assert lib.crs_encoder_plan_describe(ctypes.byref(d), 8, 513, 0, 0, None, 0) == -1      # CRS_EINVAL: seq > max_pos
