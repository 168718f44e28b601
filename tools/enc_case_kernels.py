"""Which kernels does an encoder call launch, with which grid, workgroup size and LDS?  The planner (csrc/enc_plan.cpp) says so
on a CPU -- crs_encoder_plan_describe, tools/enc_plan_table.cpp -- and tests/test_enc_plan_cpu.py holds it to
tests/golden/enc_plans.json.xz.  This tool makes that file from a device and confirms that the launch matches the plan:

    rocprofv3 --kernel-trace -d OUT -o rec --output-format csv -- python tools/enc_case_kernels.py record OUT/calls.json [full|grid]
    python tools/enc_case_kernels.py reduce OUT/calls.json OUT/rec_kernel_trace.csv > OUT/record.json
    python tools/enc_case_kernels.py golden OUT0/record.json OUT1/record.json ...   -> tests/golden/enc_plans.json.xz
    python tools/enc_case_kernels.py table > profiles/enc_cases_kernels.txt          (from the golden: kernel names per case)

`record` runs in one fresh process per knob setting (the CRS_* variables of its environment are written into calls.json):
one forward per call of calls(), each behind a marker kernel (tan_ on a 64-element tensor) so that `reduce` can cut the trace,
which is ordered by start time on the one stream used, into calls; it also asks crs_encoder_workspace_bytes for the byte
table.  Weights are zeros of the model's shape: only the dispatch matters.  `reduce` keeps, per launch, the kernel's short
name, its grid in workgroups (the trace has work-items), its workgroup size and the trace's LDS column (a kernel's STATIC LDS:
0 for the kernels that size theirs at launch, so the plan's dynamic LDS is not in this record)."""
import csv
import json
import lzma
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "compressed-rag-suite_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden", "enc_plans.json.xz")
GRID_TOKENS = [16, 64, 80, 512, 1024, 1040, 2048, 2064, 2304, 3584, 3840, 4096, 4112, 6656, 8192, 32768, 65536]   # at seq 16
GRID_SEQS = [1, 12, 16, 17, 32, 64, 65, 128, 256, 257, 512]                                                       # at batch 4
GEMMS = [(4096, 4096, 4096, 0), (8192, 8192, 8192, 0), (32768, 2304, 768, 0), (32768, 3072, 768, 1), (32768, 768, 3072, 2),
         (32768, 768, 768, 2), (65536, 1536, 384, 1), (65536, 1024, 384, 0), (4096, 2304, 768, 0), (512, 512, 768, 0),
         (512, 512, 768, 1), (511, 512, 384, 0)]
BYTES_TOKENS = list(range(16, 8193, 16)) + [t for t in GRID_TOKENS if t > 8192]


def grid_models():
    import _encoder_cases as ec
    return [("tiny", ec.TINY1), ("h128x2", ec.H128_2), ("h256x4", ec.H256_4), ("h320", ec.H320), ("minilm", ec.MINI1),
            ("h512", ec.H512), ("h640", ec.H640), ("bge", ec.BGE1), ("h1024", ec.H1024)]


def calls(scope="full"):
    """Every call of the record, as a JSON-able dict: kind fwd (hidden, heads, ffn, layers, max_pos, batch, seq, small, rel, pair)
    or gemm (m, n, k, mode).  `grid` leaves out the small-LDS, relative-bias and pair forwards."""
    import _crossenc_cases as cc
    import _encoder_cases as ec
    import _mpnet_cases as mc

    def fwd(name, cfg, batch, seq, small=0, rel=0, pair=0):
        return dict(kind="fwd", name=name, hidden=cfg.hidden, heads=cfg.heads, ffn=cfg.ffn, layers=cfg.layers, max_pos=cfg.max_pos,
                    batch=batch, seq=seq, small=small, rel=rel, pair=pair)

    out = []
    for c in ec.ALL_CASES:
        out.append(fwd("case:" + c.name, c.cfg, c.batch, c.seq))
        if c.query_batch and scope == "full":
            out.append(fwd("case:" + c.name, c.cfg, c.batch, c.seq, small=1))
    if scope == "full":
        for key, cfg, _, batch, seq in mc.CASES:
            for small in (0, 1):
                out.append(dict(fwd("mpnet:" + key, cfg, batch, seq, small=small, rel=1), max_pos=cfg.max_pos - mc.POS_OFFSET))
        for key, cfg, _, batch, seq in cc.CASES:
            out.append(fwd("crossenc:" + key, cfg, batch, seq, pair=1))
    for name, cfg in grid_models():
        out += [fwd(f"grid:{name}-T{t}", cfg, t // 16, 16) for t in GRID_TOKENS]
        out += [fwd(f"grid:{name}-4x{s}", cfg, 4, s) for s in GRID_SEQS if s <= cfg.max_pos]
    out += [dict(kind="gemm", name="gemm:%dx%dx%d-%d" % g, m=g[0], n=g[1], k=g[2], mode=g[3]) for g in GEMMS]
    return out


def zero_weights(c):
    import numpy as np
    h, f = c["hidden"], c["ffn"]
    rows = c["max_pos"] + (2 if c["rel"] else 0)
    w = {"embeddings.word_embeddings.weight": (1000, h), "embeddings.position_embeddings.weight": (rows, h),
         "embeddings.token_type_embeddings.weight": (2, h), "embeddings.LayerNorm.weight": (h,), "embeddings.LayerNorm.bias": (h,)}
    for i in range(c["layers"]):
        p = f"encoder.layer.{i}."
        for n in ("query", "key", "value"):
            w[p + f"attention.self.{n}.weight"], w[p + f"attention.self.{n}.bias"] = (h, h), (h,)
        w[p + "attention.output.dense.weight"], w[p + "attention.output.dense.bias"] = (h, h), (h,)
        w[p + "intermediate.dense.weight"], w[p + "intermediate.dense.bias"] = (f, h), (f,)
        w[p + "output.dense.weight"], w[p + "output.dense.bias"] = (h, f), (h,)
        for n in ("attention.output.LayerNorm", "output.LayerNorm"):
            w[p + n + ".weight"], w[p + n + ".bias"] = (h,), (h,)
    if c["rel"]:
        w["encoder.relative_attention_bias.weight"] = (32, c["heads"])
    if c["pair"]:
        w.update({"pooler.dense.weight": (h, h), "pooler.dense.bias": (h,), "classifier.weight": (1, h), "classifier.bias": (1,)})
    return {k: np.zeros(s, dtype=np.float32) for k, s in w.items()}


def record(path, scope):
    import torch
    from rag import _native as nat
    from rag._encoder import HipEncoder, ModelShape, gemm_f16
    dev = torch.device("cuda:0")
    m = torch.zeros(64, device=dev)
    todo = calls(scope)
    encs = {}

    def encoder(c):
        key = (c["hidden"], c["heads"], c["ffn"], c["layers"], c["max_pos"], c["rel"], c["pair"])
        if key not in encs:
            extra = dict(rel_buckets=32, pos_offset=2) if c["rel"] else {}
            shape = ModelShape(1000, c["hidden"], c["layers"], c["heads"], c["ffn"], c["max_pos"] + (2 if c["rel"] else 0), 1e-12,
                               "cls" if c["pair"] else "mean", c["max_pos"], **extra)
            encs[key] = HipEncoder(shape, zero_weights(c), device=dev)
        return encs[key]

    for c in todo:
        if c["kind"] == "gemm":
            a = torch.zeros((c["m"], c["k"]), dtype=torch.float16, device=dev)
            w = torch.zeros((c["n"], c["k"]), dtype=torch.float16, device=dev)
            bias = torch.zeros(c["n"], device=dev)
            res = torch.zeros((c["m"], c["n"]), device=dev) if c["mode"] == 2 else None
            torch.cuda.synchronize()
            m.tan_()
            gemm_f16(a, w, bias, res, c["mode"])
            torch.cuda.synchronize()
            del a, w, bias, res
            continue
        enc = encoder(c)
        ids = torch.zeros((c["batch"], c["seq"]), dtype=torch.int32, device=dev)
        lens = torch.full((c["batch"],), c["seq"], dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        m.tan_()
        if c["pair"]:
            enc.score_pairs(ids, ids, lens)
        else:
            enc.forward(ids, lens, small_lds=bool(c["small"]))
        torch.cuda.synchronize()
        if c["batch"] * c["seq"] > 8192:
            enc._ws = None
    m.tan_()
    torch.cuda.synchronize()
    # the byte table: a pure host call
    sizes = {}
    for name, cfg in grid_models():
        enc = encoder(dict(hidden=cfg.hidden, heads=cfg.heads, ffn=cfg.ffn, layers=cfg.layers, max_pos=cfg.max_pos, rel=0, pair=0))
        sizes[name] = [enc.workspace_bytes(t // 16, 16) for t in BYTES_TOKENS]
    json.dump({"env": {k: v for k, v in sorted(os.environ.items()) if k.startswith("CRS_") and k != "CRS_LIB_PATH"},
               "cus": torch.cuda.get_device_properties(0).multi_processor_count, "calls": todo, "bytes": sizes}, open(path, "w"))


def short_name(name):
    """_ZN3crs12_GLOBAL__N_117gemm_panel_kernelILi3ELi64EEEv... or void crs::(anonymous namespace)::gemm_panel_kernel<3, 64>(...)
    -> gemm_panel_kernel<3, 64> (integer / bool template arguments)."""
    m = re.match(r"_ZN3crs(?:12_GLOBAL__N_1)?(\d+)", name)
    if not m:
        name = name.replace("(anonymous namespace)::", "").replace("void ", "").replace("crs::", "")
        return re.sub(r"\(bool\)1|\(bool\)0", lambda b: "true" if b.group(0).endswith("1") else "false", name.split("(")[0]).strip()
    n = int(m.group(1))
    base, rest = name[m.end():m.end() + n], name[m.end() + n:]
    args = []
    if rest.startswith("I"):
        rest = rest[1:]
        while True:
            a = re.match(r"L([ib])(n?\d+)E", rest)
            if not a:
                break
            args.append(a.group(2).replace("n", "-") if a.group(1) == "i" else ("true" if a.group(2) == "1" else "false"))
            rest = rest[a.end():]
    return base + (f"<{', '.join(args)}>" if args else "")


def reduce(calls_path, trace_path):
    rec = json.load(open(calls_path))
    rows = list(csv.DictReader(open(trace_path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    segs, cur = [], None
    for r in rows:
        n = r["Kernel_Name"]
        if "tan" in n.lower() and "crs" not in n:
            cur = []
            segs.append(cur)
        elif cur is not None and ("crs::" in n or n.startswith("_ZN3crs")):
            wg = [int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"]
            grid = [int(r[f"Grid_Size_{a}"]) // w for a, w in zip("XYZ", wg)]
            cur.append([short_name(n), grid, wg, int(r["LDS_Block_Size"])])
    assert len(segs) == len(rec["calls"]) + 1 and not segs[-1], (len(segs), len(rec["calls"]))
    for c, s in zip(rec["calls"], segs):
        assert s, c
        c["launches"] = s
    json.dump(rec, sys.stdout)


def launch_text(l):
    name, grid, wg, lds = l
    return "%s grid=%s wg=%s lds=%d" % (name, "x".join(map(str, grid)), "x".join(map(str, wg)), lds)


def golden(paths):
    """texts: every distinct launch line; lists: every distinct launch list (indices into texts); per setting the calls
    (their fields, and the index of their list) and the byte table (indices into sizes)."""
    texts, lists, sizes, settings, cus = {}, {}, {}, [], None
    for p in paths:
        rec = json.load(open(p))
        assert cus in (None, rec["cus"])
        cus = rec["cus"]
        out = []
        for c in rec["calls"]:
            key = tuple(texts.setdefault(launch_text(l), len(texts)) for l in c.pop("launches"))
            out.append(dict(c, list=lists.setdefault(key, len(lists))))
        settings.append({"env": rec["env"], "calls": out,
                         "bytes": {k: [sizes.setdefault(b, len(sizes)) for b in v] for k, v in rec["bytes"].items()}})
    g = {"cus": cus, "bytes_tokens": BYTES_TOKENS, "texts": list(texts), "lists": [list(k) for k in lists], "sizes": list(sizes),
         "settings": settings}
    with lzma.open(GOLDEN, "wt", preset=9) as f:
        json.dump(g, f, separators=(",", ":"))


def table():
    import _encoder_cases as ec
    with lzma.open(GOLDEN, "rt") as f:
        g = json.load(f)
    dflt = next(s for s in g["settings"] if not s["env"])
    by_name = {c["name"]: c for c in dflt["calls"] if not c.get("small")}
    print(f"Kernels of ONE default forward per case of tests/_encoder_cases.py on an MI355X ({g['cus']} CUs; rocprofv3 --kernel-trace,")
    print("tools/enc_case_kernels.py; from tests/golden/enc_plans.json.xz, which tests/test_enc_plan_cpu.py holds the planner to),")
    print("in launch order, each kernel listed once.  `why` is the branch the case is in the table for.\n")
    for case in ec.ALL_CASES:
        print(f"{case.name}  [{case.cfg.hidden} / {case.cfg.heads} heads / ffn {case.cfg.ffn} / {case.cfg.layers} layer(s), {case.batch} x {case.seq}]  why: {case.why}")
        seen = []
        for i in g["lists"][by_name["case:" + case.name]["list"]]:
            k = g["texts"][i].split(" grid=")[0]
            if k not in seen:
                seen.append(k)
        for k in seen:
            print("    " + k)


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "record":
        record(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else "full")
    elif mode == "reduce":
        reduce(sys.argv[2], sys.argv[3])
    elif mode == "golden":
        golden(sys.argv[2:])
    else:
        table()
