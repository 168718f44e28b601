"""No GPU: the bound of tests/_gemm_ref.py discriminates.  An fp32 emulation of the kernels' accumulation order stays inside it at
EVERY element, and each of six planted faults -- the kinds of error a tile kernel commits at a ragged edge, each a few 1e-3 to 1e-1
in one projection -- exceeds it in at least one element, in every mode it applies to.  Also: the four test-facing entries
(crs_gemm_f16_routed, crs_gemm_plan_describe, crs_proj_ln_f16, crs_proj_ln_plan_describe) are declared, exported and bound, and
the describe entries and the planner answer what the GPU tests' tables expect at 256 CUs."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _gemm_cases as gc  # noqa: E402
import _gemm_ref as gr  # noqa: E402

# two small shapes: ragged last row tile (200 = 128 + 72, 300 = 2 x 128 + 44), N no multiple of 8 / of the 64- and 128-column
# blocks, K short enough that E stays below the tanh-GELU's 2e-4 and long enough for 2 / 3 slabs of whole 64-column chunks
SHAPES = [(200, 77, 128, 2), (300, 160, 192, 3)]


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s[:3])))
def drawn(request):
    m, n, k, slabs = request.param
    a, w, bias, res = gr.make_inputs(m, n, k)
    refs = {mode: gr.gemm_ref_and_bound(a, w, bias, res, mode, slabs) for mode in (0, 1, 2, 3)}
    return a, w, bias, res, slabs, refs


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_fp32_emulation_is_inside_the_bound_everywhere(drawn, mode):
    a, w, bias, res, slabs, refs = drawn
    ref, bound = refs[mode]
    for step in (16, 64):                     # one MFMA's depth; a whole 64-column k-tile summed before it meets the accumulator
        out = gr.emulate(a, w, bias, res, mode, slabs, step=step)
        r = gr.ratio(out, ref, bound)
        print(f"emulation mode {mode} step {step}: max err / bound = {r:.3f}")
        assert out.shape == ref.shape and r <= 1.0
    if mode != 3:                             # without a bias the bias term is gone
        ref0, bound0 = gr.gemm_ref_and_bound(a, w, None, res, mode)
        assert gr.ratio(gr.emulate(a, w, None, res, mode), ref0, bound0) <= 1.0


@pytest.mark.parametrize("fault,mode", [(f, m) for f, modes in gr.FAULTS.items() for m in modes])
def test_every_planted_fault_exceeds_the_bound(drawn, fault, mode):
    a, w, bias, res, slabs, refs = drawn
    ref, bound = refs[mode]
    out = gr.emulate(a, w, bias, res, mode, slabs, fault=fault)
    bad = ((out.double() - ref).abs() > bound)
    print(f"{fault} mode {mode}: {int(bad.sum())} elements outside, max err / bound = {gr.ratio(out, ref, bound):.1f}")
    assert bad.any()
    # ... and only where the fault was planted: the rest of the matrix stays inside
    clean = gr.emulate(a, w, bias, res, mode, slabs)
    same = (out == clean) if out.dtype != torch.float16 else (out.view(torch.int16) == clean.view(torch.int16))
    assert not (bad & same).any()


def test_half_ulp_is_subnormal_aware():
    x = torch.tensor([1.0, 1.999, 2.0, 2.0 ** -14, 2.0 ** -15, 0.0, 6e-8], dtype=torch.float64)
    want = torch.tensor([2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -25, 2.0 ** -25, 2.0 ** -25, 2.0 ** -25], dtype=torch.float64)
    assert torch.equal(gr.half_ulp16(x), want)


def test_proj_ln_bound_is_first_order_and_catches_a_dropped_slab_chunk():
    """The LayerNorm propagation: an fp32 emulation (chunked accumulation, torch's fp32 LayerNorm) is inside; the second-order term is
    below 1 % of the bound; 16 dropped K columns in the last ragged row tile are outside."""
    t, h, k = 200, 384, 192
    a, w, bias, res = gr.make_inputs(t, h, k)
    gen = torch.Generator().manual_seed(5)
    g, b = 1.0 + 0.1 * torch.randn(h, generator=gen), 0.1 * torch.randn(h, generator=gen)
    for slabs in (1, 3):
        ref, b32, b16, second, a_term = gr.proj_ln_ref_and_bound(a, w, bias, res, g, b, 1e-12, slabs)
        assert second < 0.01
        for fault in (None, "drop_last_k16"):
            y = sum(gr.emulate(a, w, None, None, 3, slabs, fault=fault)) + bias[None, :] + res
            out = torch.nn.functional.layer_norm(y, (h,), g, b, 1e-12)
            r32, r16 = gr.ratio(out, ref, b32), gr.ratio(out.half(), ref, b16)
            print(f"proj_ln slabs {slabs} fault {fault}: x32 {r32:.3f} x16 {r16:.3f} (second order {second:.1e}, a {a_term:.1e})")
            assert (r32 <= 1.0 and r16 <= 1.0) if fault is None else (r32 > 1.0 and r16 > 1.0)


# ---- the entries --------------------------------------------------------------------------------------------------------------------
ENTRIES = ("crs_gemm_f16_routed", "crs_gemm_plan_describe", "crs_proj_ln_f16", "crs_proj_ln_plan_describe")


def test_entries_are_declared_exported_and_bound():
    from rag import _encoder as enc
    from rag import _native as nat
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crs_encoder.h")).read(), flags=re.S)
    lib = nat.load()
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, header), f"{name} not declared in include/crs_encoder.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in nat.exported_symbols()
    assert lib.crs_abi_version() == 3
    for fn in ("gemm_f16_routed", "gemm_plan_describe", "proj_ln_f16", "proj_ln_plan_describe"):
        assert callable(getattr(enc, fn))
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert name in text, f"{name} not documented in INTEGRATION.md"


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "enc_plan_table")
    csrc = os.path.join(ROOT, "compressed-rag-suite_amd", "csrc")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tools", "enc_plan_table.cpp"),
                    os.path.join(csrc, "enc_plan.cpp")], check=True, timeout=300)

    def run(lines, env):
        e = {k: v for k, v in os.environ.items() if not k.startswith("CRS_")}
        e.update(env)
        r = subprocess.run([exe, str(gc.TABLE_CUS)], input="".join(" ".join(map(str, c)) + "\n" for c in lines), env=e, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        rows = []
        for line in r.stdout.splitlines():      # "gemm=Family/slabs/tm/kc/kin/... <tab> describe lines joined by ';'"
            fields, text = line.split("\t")
            plan = re.search(r"gemm=(\w+)/(\d+)/(\d+)/(\d+)/(\d+)/", fields).groups()
            rows.append((plan[0],) + tuple(map(int, plan[1:])) + (text.rstrip(";").split(";"),))
        return rows
    return run


def test_the_planner_gives_every_case_the_kernel_it_names(table):
    """What crs_gemm_plan_describe / crs_proj_ln_plan_describe will answer on a 256-CU device, from the planner alone: every case of
    the GPU tests' tables names the kernel (with template arguments) the planner picks under its setting, and the slab counts."""
    assert len(gc.SETTINGS) <= 10 + 1 and gc.SETTINGS[0] == {}
    chunks = set()
    for si, setting in enumerate(gc.SETTINGS):
        cases = [c for c in gc.GEMM_CASES if c.setting == si]
        got = table([("route", c.m, c.n, c.k, c.mode, c.route, c.flags) for c in cases], setting)
        for c, (family, slabs, tm, kc, kin, text) in zip(cases, got):
            assert len(text) == 1 and text[0].startswith(c.kernel + " grid="), (setting, c, text)
            assert slabs == c.slabs, (setting, c, slabs)
            if c.mode == 3:
                assert gc.slab_factor(c, text[0]) == c.slabs, (setting, c, text)
            if c.family == "gemm8p":
                assert gc.grid_of(text[0]) == (gc.TABLE_CUS, 1, 1) and (c.m // 256) * ((c.n + 255) // 256) % gc.TABLE_CUS in (1, 2, 3, 4)
            if family == "Panel":
                assert kc * kin * slabs == c.k
                chunks.add((c.mode == 3, kc, kin > 1))
        pcases = [c for c in gc.PROJ_LN_CASES if c.setting == si]
        got = table([("projln", c.tokens, c.hidden, c.k, c.flags, int(c.big_ln)) for c in pcases], setting)
        for c, (family, slabs, tm, kc, kin, text) in zip(pcases, got):
            assert [t.split(" grid=")[0] for t in text] == list(c.kernels), (setting, c, text)
            assert slabs == c.slabs
    used = {c.setting for c in gc.GEMM_CASES} | {c.setting for c in gc.PROJ_LN_CASES}
    assert used == set(range(len(gc.SETTINGS)))
    # the panel kernel's staging: one-shot 384 / 256 / 128-column chunks and chunks walked kin > 1 times, in fp16 and slab modes
    for want in [(False, 384, False), (False, 128, True), (False, 256, False), (False, 128, False), (True, 384, False), (True, 384, True),
                 (True, 128, True), (False, 384, True)]:
        assert want in chunks, (want, sorted(chunks))


def test_the_table_reaches_every_family_and_branch():
    kernels = {c.kernel for c in gc.GEMM_CASES}
    for want in ("gemm_f16_kernel<0>", "gemm_f16_kernel<1>", "gemm_f16_kernel<2>", "gemm_panel_kernel<0, 64>", "gemm_panel_kernel<1, 128>",
                 "gemm_panel_kernel<3, 64>", "gemm_panel_kernel<3, 128>", "gemm8_kernel<0, false, 0>", "gemm8_kernel<1, true, 0>",
                 "gemm8_kernel<2, false, 0>", "gemm8_kernel<3, false, 0>", "gemm8_kernel<0, false, 1>", "gemm8_kernel<0, false, 2>",
                 "gemm8_kernel<0, false, 3>", "gemm_big_kernel<0, 256>", "gemm_big_kernel<1, 256>", "gemm_stream_kernel<128, 0>",
                 "gemm_stream_kernel<512, 1>", "gemm_stream_ks_kernel<768, 0>", "gemm_stream_ks_kernel<768, 1>"):
        assert want in kernels, want
    # odd N and N that is no multiple of 8 on the tiled kernel (the epilogue guards), N % 8 != 0 and N % 4 != 0 on the panel kernel
    assert any(c.kernel.startswith("gemm_f16_kernel") and c.n % 2 for c in gc.GEMM_CASES)
    assert any(c.kernel.startswith("gemm_panel_kernel<3") and c.n % 4 for c in gc.GEMM_CASES)
    # the pipelined kernel at k-step counts that are no multiple of its four stages
    assert any(c.kernel.startswith("gemm_big") and (c.k // 32) % 4 for c in gc.GEMM_CASES)
    lines = {k for c in gc.PROJ_LN_CASES for k in c.kernels}
    for want in ("gemm_rowln2_kernel<64, 2>", "gemm_rowln2_kernel<32, 4>", "gemm_panel_kernel<3, 64>", "gemm8_kernel<3, false, 0>",
                 "gemm_f16_kernel<2>", "layernorm_kernel<16, 1>", "layernorm2_kernel<3, 4>", "layernorm2_kernel<6, 2>", "layernorm2_kernel<6, 3>"):
        assert want in lines, want
