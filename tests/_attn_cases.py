"""The case table of tests/test_attn_forms_gpu.py and tests/test_attn_ref_cpu.py: every attention kernel instantiation the encoder can
launch (csrc/enc_attn.hip: 17 names, the bias forms included; csrc/enc_qkvattn.hip: 2), each case naming the kernel with template
arguments it must run and the route (crs_attention_f16) that reaches it.  Shapes are the smallest that still exercise each edge:
sequence lengths around the 16-key tile, the 64-key block and the 256 / 512-token LDS images; 2 or 3 heads (12 where the fused kernel's
hidden 384 at head_dim 32 needs them); 5 to 9 batch rows (3 for the fused kernel's 3 x 64 tokens).  The lens of a case are 1, 0 (clamped
to 1), seq + 5 (clamped to seq), the inner lengths written out in the table below, and seq in the last row; a batch holds a few inner
lengths, so the boundary values of a form -- 16 / 17, 63 / 64 / 65, 128 / 129 for the blocked kernels, lengths inside a 32-key group and
at the 64 / 128 / 256 block boundaries for the whole-sequence ones -- are SPREAD over the form's cases, and REQUIRED_LENS states which
values every form (and every whole-sequence instantiation) must hold; tests/test_attn_ref_cpu.py asserts it."""
from collections import namedtuple

RATIO_TAG = "attn-ratio"
ROUTE_FUSED = 16            # crs_attention_plan_describe: the launch of crs_qkv_attn_f16

# form: blocked | bias | short | seq | seq32 | fused (the emulation's form and the profile's family); span: 0 without a bias;
# hidden = heads * hd
AttnCase = namedtuple("AttnCase", "form kernel hd heads batch seq lens route peaked span seed")


def attn_id(c):
    return (f"{c.form}-hd{c.hd}-h{c.heads}-b{c.batch}-s{c.seq}-r{c.route}" + ("-peaked" if c.peaked else "") + (f"-span{c.span}" if c.span else ""))


def lens_for(seq, inner):
    """1, 0, seq + 5, the inner lengths, and seq LAST: the last batch row's keys reach the sequence's last block, whose rows >= seq lie
    behind the tensor.  Every inner length must be one (1 < len < seq): none is dropped silently."""
    assert all(1 < e < seq for e in inner) and len(set(inner)) == len(inner), (seq, inner)
    return (1, 0, seq + 5) + tuple(inner) + (seq,)


def _case(form, kernel, hd, heads, seq, route, inner, peaked=False, span=0):
    lens = lens_for(seq, inner)
    batch = len(lens)
    seed = 1000 * hd + 7 * seq + heads + 31 * batch          # the input depends on the shape alone: routes share it
    return AttnCase(form, kernel, hd, heads, batch, seq, lens, route, peaked, span, seed)


# inner lengths per sequence length (the batch is 4 + their count)
BLOCKED_LENS = {1: (), 15: (2, 7, 14), 17: (2, 8, 15, 16), 48: (16, 17, 32, 33, 47), 64: (16, 17, 32, 48, 63), 65: (16, 17, 33, 63, 64),
                130: (63, 64, 65, 128, 129), 300: (16, 17, 128, 129, 257)}
BLOCKED_LENS_PEAKED = {64: (15, 31, 33, 49, 62), 130: (16, 17, 64, 127, 129), 300: (63, 65, 192, 256, 299)}
BIAS_LENS = {5: (2, 3, 4), 64: (16, 17, 32, 63), 65: (16, 17, 63, 64), 130: (64, 65, 128, 129), 512: (128, 129, 449)}
SHORT_LENS = {1: (), 2: (), 5: (2, 3, 4), 12: (4, 8, 11), 16: (4, 8, 9, 12, 15)}
# whole sequence: (heads, inner lengths) per seq; heads x batch is 16 (the XCD pairing permutes the units) at 65, 150, 257, 470 and 27 at
# the others.  70, 81, 97 / 270, 289, 321: inside a 32-key group; 64, 128, 192, 256, 320, 384: block boundaries
WHOLE_256 = {65: (2, (17, 33, 63, 64)), 100: (3, (64, 65, 70, 81, 97)), 150: (2, (70, 97, 128, 129)), 256: (3, (64, 128, 129, 192, 200))}
WHOLE_512 = {257: (2, (128, 129, 200, 256)), 300: (3, (64, 256, 257, 270, 289)), 470: (2, (128, 321, 384, 449)),
             512: (3, (129, 256, 320, 449, 500))}
# fused: (batch rows, inner lengths) per seq -- a block tail (7 x 16, 5 x 32, 3 x 64 tokens) and full blocks
FUSED = {16: ((7, (2, 8, 15)), (8, (3, 5, 9, 15))), 32: ((5, (17,)), (6, (16, 31))), 64: ((3, None), (6, (33, 63)))}

# what every form's table must hold (tests/test_attn_ref_cpu.py); for seq and seq32: what every instantiation's cases must hold
REQUIRED_LENS = {"blocked": {16, 17, 63, 64, 65, 128, 129}, "bias": {16, 17, 63, 64, 65, 128, 129},
                 "whole_256": {64, 128, 70, 81, 97}, "whole_512": {64, 128, 256, 270, 289, 321}}


def _build():
    cases = []
    # ---- blocked, plain: route 2 keeps hd 32 / 64 off the short kernel up to 16 tokens; route 1 keeps 65 .. off the whole-sequence ones
    for hd in (16, 32, 64):
        for seq, inner in BLOCKED_LENS.items():
            if seq <= 16:
                route = 0 if hd == 16 else 2
            elif seq <= 64:
                route = 0
            else:
                route = 0 if (seq == 300 and hd == 32) else 1
            heads = 3 if seq in (130, 300) else 2
            cases.append(_case("blocked", f"attention_kernel<{hd}, false>", hd, heads, seq, route, inner))
            if seq in BLOCKED_LENS_PEAKED:
                cases.append(_case("blocked", f"attention_kernel<{hd}, false>", hd, heads, seq, route, BLOCKED_LENS_PEAKED[seq], True))
    # ---- blocked, with a relative-position bias: span = seq and seq + 7 at every length
    for hd in (16, 32, 64):
        for seq, inner in BIAS_LENS.items():
            for span in (seq, seq + 7):
                cases.append(_case("bias", f"attention_kernel<{hd}, true>", hd, 2 if seq == 512 else 3, seq, 0, inner, False, span))
    # ---- short: one wave per (sequence, head), four per workgroup: units a multiple of 4 (seq 1 and 2: four batch rows) and not (the
    # `unit >= n_units` tail: 2 or 3 heads x 7 or 9 rows = 14, 18, 21, 27 units at seq 5, 12, 16)
    for hd in (32, 64):
        for i, (seq, inner) in enumerate(SHORT_LENS.items()):
            heads = (2, 3)[(i + hd // 32) % 2]
            cases.append(_case("short", f"attention_short_kernel<{hd}>", hd, heads, seq, 0, inner))
    # ---- whole sequence, 16-deep (route 4, or head_dim 16) and 32-deep (QT 4: route 8)
    def whole(form, name, hd, table, route):
        for seq, (heads, inner) in table.items():
            cases.append(_case(form, name, hd, heads, seq, route, inner))
    whole("seq", "attention_seq_kernel<32, 256, 4>", 32, WHOLE_256, 4)
    whole("seq", "attention_seq_kernel<16, 256, 4>", 16, WHOLE_256, 0)
    whole("seq", "attention_seq_kernel<64, 256, 4>", 64, WHOLE_256, 4)
    whole("seq", "attention_seq_kernel<64, 512, 8>", 64, WHOLE_512, 4)
    whole("seq32", "attention_seq32_kernel<32, 256, 4, 2>", 32, WHOLE_256, 0)
    whole("seq32", "attention_seq32_kernel<64, 256, 4, 2>", 64, WHOLE_256, 0)
    whole("seq32", "attention_seq32_kernel<32, 256, 4, 4>", 32, WHOLE_256, 8)
    whole("seq32", "attention_seq32_kernel<64, 512, 8, 2>", 64, WHOLE_512, 0)
    whole("seq32", "attention_seq32_kernel<64, 512, 8, 4>", 64, WHOLE_512, 8)
    # ---- fused QKV projection + attention: 64-token blocks
    for hd, hidden in ((32, 128), (32, 256), (32, 384), (64, 128)):
        for seq, variants in FUSED.items():
            for batch, inner in variants:
                c = _case("fused", f"qkv_attn_kernel<{hd}>", hd, hidden // hd, seq, ROUTE_FUSED, inner or ())
                if inner is None:        # 3 x 64 tokens: three rows hold 1, 0 and seq
                    c = c._replace(batch=3, lens=(1, 0, seq), seed=c.seed - 31)
                assert c.batch == batch
                cases.append(c)
    return cases


CASES = _build()

# every instantiation the forward can launch: 19 distinct kernel names
INSTANTIATIONS = tuple([f"attention_kernel<{hd}, {b}>" for hd in (16, 32, 64) for b in ("false", "true")] +
                       ["attention_short_kernel<32>", "attention_short_kernel<64>",
                        "attention_seq_kernel<32, 256, 4>", "attention_seq_kernel<16, 256, 4>", "attention_seq_kernel<64, 512, 8>",
                        "attention_seq_kernel<64, 256, 4>",
                        "attention_seq32_kernel<32, 256, 4, 4>", "attention_seq32_kernel<64, 512, 8, 4>",
                        "attention_seq32_kernel<32, 256, 4, 2>", "attention_seq32_kernel<64, 512, 8, 2>",
                        "attention_seq32_kernel<64, 256, 4, 2>", "qkv_attn_kernel<32>", "qkv_attn_kernel<64>"])


def expected_grid(c):
    """the describe line's grid, from batch, heads and seq alone"""
    if c.form in ("blocked", "bias"):
        return ((c.seq + 63) // 64, c.heads, c.batch)
    if c.form == "short":
        return ((c.heads * c.batch + 3) // 4, 1, 1)
    if c.form == "fused":
        return ((c.batch * c.seq + 63) // 64, c.heads, 1)
    return (c.heads * c.batch, 1, 1)


def grid_of(text):
    return tuple(int(x) for x in text.split(" grid=")[1].split()[0].split("x"))


# ---- inputs and fp64 references, computed once per distinct input and shared by the cases (routes, launches) that use it ---------------
_refs = {}


def case_inputs(c):
    """blocked .. seq32: (qkv fp16 [T, 3H], bias fp32 [heads, 2 span - 1] or None); fused: (x16, w, b_qkv)"""
    import _attn_ref as ar
    if c.form == "fused":
        return ar.make_fused_inputs(c.batch, c.seq, c.heads * c.hd, c.heads, c.lens, c.seed)
    return ar.make_inputs(c.batch, c.seq, c.heads, c.hd, c.lens, c.seed, c.peaked), (ar.make_bias(c.heads, c.span, c.seed + 1) if c.span else None)


def case_reference(c):
    """(inputs, ref, bound, info); at most four inputs are kept: cases that share one are neighbours in the table"""
    import _attn_ref as ar
    key = (c.form == "fused", c.hd, c.heads, c.batch, c.seq, c.lens, c.peaked, c.span, c.seed)
    if key not in _refs:
        if len(_refs) >= 4:
            _refs.pop(next(iter(_refs)))
        inp = case_inputs(c)
        if c.form == "fused":
            _refs[key] = (inp,) + ar.fused_ref_and_bound(inp[0], inp[1], inp[2], c.lens, c.batch, c.seq, c.heads)
        else:
            _refs[key] = (inp,) + ar.ref_and_bound(inp[0], c.lens, c.batch, c.seq, c.heads, c.hd, inp[1])
    return _refs[key]
