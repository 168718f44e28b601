"""No GPU: the bounds of tests/_row_ref.py discriminate.  An fp32 numpy emulation of every row kernel in the kernel's summation order --
the lane-strided LayerNorm forms with the wave butterfly, the pooling kernel's four waves x four unrolled accumulators with the stride-4
tail, the pair head's lane-strided dot products and per-wave classifier sums -- stays inside them at EVERY case of tests/_row_cases.py,
and each planted fault leaves them at the cases designed for that fault.  Also: the five test-facing entries (crs_embed_ln_f32,
crs_layernorm_f32, crs_pool_f32, crs_pair_head_f32, crs_row_plan_describe) are declared, exported, bound and documented;
crs_row_plan_describe answers without a device, names the instantiation and grid of every case, and gives the line the forward's plan
prints (tools/enc_plan_table.cpp) wherever a forward of the same sizes launches the kernel."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _row_cases as rc  # noqa: E402
import _row_ref as rr  # noqa: E402


@pytest.mark.parametrize("c", rc.ALL_CASES, ids=rc.case_id)
def test_fp32_emulation_is_inside_the_bound_at_every_case(c):
    _, ref = rc.case_reference(c)
    if isinstance(c, (rc.EmbedCase, rc.LnCase)):
        assert ref[3] < rr.SECOND_ORDER_LIMIT, f"inadmissible case: second-order term {ref[3]:.2e} of the bound"
    outs = rc.emulate(c)
    print(f"emulation {c.id}: " + ", ".join(f"{k} {v:.3f}" for k, v in rc.ratios(c, outs).items()))
    assert rc.violations(c, outs) == []


# ---- planted faults: fault -> the cases designed for it -----------------------------------------------------------------------------------
FAULT_CASES = {
    "pos_row_t": [c for c in rc.EMBED_CASES if c.pos and c.tokens > rc.SEQ],
    "type_row_ignored": [c for c in rc.EMBED_CASES if c.typed and c.type_rows == 2],
    "uncentred_variance": [c for c in rc.LN_CASES if c.tokens >= 5],
    "one_pass_variance": [c for c in rc.LN_CASES if c.big_row is not None],
    "eps_outside_sqrt": [c for c in rc.LN_CASES if c.eps == 1e-5 and c.tokens >= 5],
    "mean_over_64pl": [c for c in rc.LN_CASES if c.hidden in (128, 320)],
    "last_slab_dropped": [c for c in rc.LN_CASES if c.nsplit >= 2],
    "bias_skipped": [c for c in rc.LN_CASES if c.bias],
    "residual_skipped": [c for c in rc.LN_CASES if c.residual],
    "mean_over_seq": [c for c in rc.POOL_CASES if c.pooling == 0 and not c.normalize],      # (normalised, the factor cancels: no fault)
    "last_token_dropped_at_13_mod_16": [c for c in rc.POOL_CASES if c.pooling == 0],
    "token_len_included": [c for c in rc.POOL_CASES if c.pooling == 0],
    "cls_reads_last_token": [c for c in rc.POOL_CASES if c.pooling == 1],
    "padding_unwritten": [c for c in rc.POOL_CASES if c.pdim16 > c.hidden],
    "pooler_bias_skipped": rc.PAIR_CASES,
    "tanh_skipped": rc.PAIR_CASES,
    "sigmoid_skipped": [c for c in rc.PAIR_CASES if c.activation == 1],
    "neighbour_cls_row": [c for c in rc.PAIR_CASES if c.batch >= 7],
    "token_1_read": [c for c in rc.PAIR_CASES if c.seq == 3],
}


def test_every_fault_has_cases_in_every_form_it_applies_to():
    assert set(FAULT_CASES) == set(rr.EMBED_FAULTS + rr.LN_FAULTS + rr.POOL_FAULTS + rr.PAIR_FAULTS)
    assert all(FAULT_CASES.values())
    forms = lambda f: {c.kernel.split("<")[0] + "<" + c.kernel.split("<")[1].split(",")[0] for c in FAULT_CASES[f]}
    ln_forms = {"layernorm_kernel<1", "layernorm_kernel<16", "layernorm2_kernel<3", "layernorm2_kernel<6"}
    for f in ("uncentred_variance", "one_pass_variance", "eps_outside_sqrt", "last_slab_dropped", "bias_skipped", "residual_skipped"):
        assert forms(f) == ln_forms, f
    assert forms("mean_over_64pl") == {"layernorm_kernel<16"}
    for f in ("pos_row_t", "type_row_ignored"):
        assert {c.hidden for c in FAULT_CASES[f]} == set(rc.HIDDENS), f
    assert {c.pdim16 - c.hidden for c in FAULT_CASES["padding_unwritten"]} >= {64, 192, 128}
    for f in rr.PAIR_FAULTS:
        assert {c.kernel for c in FAULT_CASES[f]} == {"pair_head_kernel<1>", "pair_head_kernel<2>"}, f


@pytest.mark.parametrize("fault,c", [(f, c) for f in FAULT_CASES for c in FAULT_CASES[f]], ids=lambda v: v if isinstance(v, str) else v.id)
def test_every_planted_fault_leaves_the_bound(fault, c):
    outs = rc.emulate(c, fault=fault)
    bad = rc.violations(c, outs)
    print(f"{fault} {c.id}: {bad}")
    assert bad


# ---- the tables --------------------------------------------------------------------------------------------------------------------------
def test_the_tables_launch_every_instantiation_and_hold_what_they_must():
    assert {c.kernel for c in rc.ALL_CASES} == set(rc.INSTANTIATIONS) and len(rc.INSTANTIATIONS) == 8 + 28 + 1 + 2
    assert len({c.id for c in rc.ALL_CASES}) == len(rc.ALL_CASES)
    # embedding: six hidden sizes, typed with 1 and 2 rows and untyped, with and without a position table, 15 tokens and 1
    for h in rc.HIDDENS:
        mine = [c for c in rc.EMBED_CASES if c.hidden == h]
        assert {(c.typed, c.type_rows) for c in mine} == {(False, 1), (True, 1), (True, 2)} and {c.pos for c in mine} == {True, False}
        assert {c.tokens for c in mine} == {15, 1}
    ids = set(rc.EMBED_IDS)
    assert ids >= {0, rc.VOCAB - 1, 2 ** 31 - 1} and min(ids) < 0 and any(rc.VOCAB <= i < 2 ** 31 - 1 for i in ids)
    assert min(rc.EMBED_TYPE_IDS) < 0 and max(rc.EMBED_TYPE_IDS) >= 2 and len(rc.EMBED_IDS) == 15 == 3 * rc.SEQ
    # LayerNorm: every hidden size x slab count; per row form every token count, bias / residual combination and eps
    assert {(c.hidden, c.nsplit) for c in rc.LN_CASES} == {(h, ns) for h in rc.HIDDENS for ns in rc.LN_SLABS}
    for form in (1, 16, 3, 6):
        mine = [c for c in rc.LN_CASES if rr.row_form(c.hidden)[0] == form]
        assert {c.tokens for c in mine} == {1, 5, 130}, form
        assert {(c.bias, c.residual) for c in mine} == {(False, False), (False, True), (True, False), (True, True)}, form
        assert {c.eps for c in mine} == {1e-12, 1e-5}, form
        assert any(c.half_row is not None for c in mine) and any(c.big_row is not None for c in mine), form
    # pool: every length once, clamping both ways; both pdim16 of the issue
    assert set(rc.POOL_LENS) >= {0, 1, 12, 13, 15, 16, 17, 28, 29, 31, 32, 33, 40, 47, -3} and len(set(rc.POOL_LENS)) == len(rc.POOL_LENS)
    assert rc.PoolCase(64, 0, True, 1).pdim16 == 256 and rc.PoolCase(320, 0, True, 1).pdim16 == 512
    assert len(rc.POOL_CASES) == 5 * 2 * 2 * 3
    # pair head: per VEC both seq, both activations, pooled_out absent and given, a batch that is no multiple of the group with seq 3
    for vec in (1, 2):
        mine = [c for c in rc.PAIR_CASES if c.kernel == f"pair_head_kernel<{vec}>"]
        assert {c.seq for c in mine} == {1, 3} and {c.activation for c in mine} == {0, 1} and {c.pooled_out for c in mine} == {True, False}
        assert {c.batch for c in mine} == {1, 7, 8, 9, 17} and any(c.batch % rc.PAIR_GROUP and c.seq == 3 for c in mine)


def test_the_inputs_are_what_the_cases_say():
    x, lens = rc.pool_inputs(64)
    nan = x.view(torch.int32) == rr.NAN32
    for i, n in enumerate(rc.POOL_LENS):
        k = max(min(max(n, 0), rc.POOL_SEQ), 1)
        assert not nan[i, :k].any() and nan[i, k:].all()
    c = next(c for c in rc.LN_CASES if c.half_row is not None and c.nsplit >= 2)
    (y, bias, res, g, b), ref = rc.case_reference(c)
    v = rr.sum_ref_and_err(rr.ln_terms(y, bias, res))[0]
    assert (v[c.half_row] == 0.5).all() and abs(v[c.big_row].mean().item() - 100) < 0.01 and 0.005 < v[c.big_row].std().item() < 0.02
    assert torch.equal(ref[0][c.half_row], b.double())
    h = rc.pair_hidden(64, 3, 3)
    assert (h.view(torch.int32)[:, 1:] == rr.NAN32).all() and torch.isfinite(h[:, 0]).all()
    w_pool, b_pool, w_cls, b_cls = rc.pair_weights(64)
    pre = h[:, 0].double() @ w_pool.double().T + b_pool.double()
    assert pre.max() > 15 and pre.min() < -15
    for t in (w_pool, b_pool, w_cls, *rc.embed_tables(64)):
        assert torch.unique(t).numel() == t.numel()


# ---- the entries -------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("crs_embed_ln_f32", "crs_layernorm_f32", "crs_pool_f32", "crs_pair_head_f32", "crs_row_plan_describe")


def test_entries_are_declared_exported_bound_and_documented():
    from rag import _encoder as enc
    from rag import _native as nat
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crs_encoder.h")).read(), flags=re.S)
    lib = nat.load()
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, header), f"{name} not declared in include/crs_encoder.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in nat.exported_symbols()
    assert lib.crs_abi_version() == 3
    for fn in ("embed_ln_f32", "layernorm_f32", "pool_f32", "pair_head_f32", "row_plan_describe"):
        assert callable(getattr(enc, fn))
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert name in text, f"{name} not documented in INTEGRATION.md"
    for h in (64, 320, 384, 768, 1024):
        for st in (nat.SLAB_F16, nat.SLAB_I8):
            assert nat.padded_dim(h, st) == rc.padded_dim(h, st)


def test_describe_needs_no_device_and_names_every_case():
    from rag import _encoder as enc
    from rag import _native as nat
    for c in rc.ALL_CASES:
        assert enc.row_plan_describe(*c.describe) == c.line, c
    for bad in ((4, 8, 384, 0), (-1, 8, 384, 0), (0, 0, 384, 0), (2, 0, 384, 0), (3, -1, 384, 0), (0, 8, 0, 0), (0, 8, 100, 0),
                (0, 8, 1088, 0), (1, 8, 384, 0), (1, 8, 384, 5), (1, 8, 384, 7), (1, 8, 384, 32)):
        with pytest.raises(nat.NativeError):
            enc.row_plan_describe(*bad)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("row_plan") / "enc_plan_table")
    csrc = os.path.join(ROOT, "compressed-rag-suite_amd", "csrc")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tools", "enc_plan_table.cpp"),
                    os.path.join(csrc, "enc_plan.cpp")], check=True, timeout=300)

    def run(lines):
        e = {k: v for k, v in os.environ.items() if not k.startswith("CRS_")}
        r = subprocess.run([exe, "256"], input="".join(" ".join(map(str, c)) + "\n" for c in lines), env=e, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        return [[t + "\n" for t in line.split("\t")[1].split(";") if t] for line in r.stdout.splitlines()]
    return run


def test_the_forward_plans_the_line_the_entry_describes(table):
    """enc_plan_describe (through tools/enc_plan_table.cpp: fwd hidden heads ffn flags batch seq rel_bias pair) for a forward of a case's
    sizes prints the line crs_row_plan_describe answers: the embedding's first, the tail's last, and the LayerNorm's with the slab
    count the forward's plan chose."""
    from rag import _encoder as enc
    fwd = lambda h, batch, seq, pair: ("fwd", h, h // 64, 4 * h, 0, batch, seq, 0, pair)
    emb = [c for c in rc.EMBED_CASES if c.tokens == 3 * rc.SEQ]
    for c, lines in zip(emb, table([fwd(c.hidden, 3, rc.SEQ, 1 if c.typed else 0) for c in emb])):
        assert lines[0] == c.line == enc.row_plan_describe(*c.describe), (c, lines)
    pool = [c for c in rc.POOL_CASES if c.pooling == 0 and c.normalize and c.out16 < 0]
    for c, lines in zip(pool, table([fwd(c.hidden, c.batch, rc.POOL_SEQ, 0) for c in pool])):
        assert lines[-1] == c.line == enc.row_plan_describe(*c.describe), (c, lines)
    for c, lines in zip(rc.PAIR_CASES, table([fwd(c.hidden, c.batch, c.seq, 2) for c in rc.PAIR_CASES])):
        assert lines[-1] == c.line == enc.row_plan_describe(*c.describe), (c, lines)
    seen = set()
    for c, lines in zip(rc.LN_CASES, table([fwd(c.hidden, c.tokens, 1, 0) for c in rc.LN_CASES])):
        planned = [t for t in lines if t.startswith("layernorm")]
        assert planned, (c, lines)
        for t in planned:
            ns = int(t.split(">")[0].split(", ")[1])
            assert t == enc.row_plan_describe(rc.KIND_LN, c.tokens, c.hidden, ns), (c, t)
            seen.add(t.split(" grid=")[0])
    print(f"LayerNorm instantiations a forward of the cases' sizes plans: {sorted(seen)}")
