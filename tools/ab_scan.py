#!/usr/bin/env python3
"""A/B of the scan kernels (csrc/scan*.hip, csrc/scan_stream.h) between two builds of the libraries: same bits, same speed.

  python tools/ab_scan.py compare LIBDIR_A LIBDIR_B [--out FILE]
  python tools/ab_scan.py time    LIBDIR_A LIBDIR_B [--rounds 5] [--launches 300] [--out profiles/scan_stream_ab.txt]

A LIBDIR holds libcrs_hip.so and libcrs_torch.so of one build.  Every measurement runs in a fresh child process that loads that
build through CRS_LIB_PATH, one child at a time (this process does not open the GPU), each under its own `timeout`; the first
child that ends with a non-zero status ends the run with that status.

compare  both builds run every case of tests/_scan_form_cases.py exactly as tests/test_scan_forms_gpu.py runs it -- all 166 forms
         with their smallest-k, ticketed, id_base and second-shape launches and their checks against fp64; the default-knob and
         CRS_WIDE_MFMA legs in one child, CRS_SCAN_TB=0, CRS_SCAN_WIDE=0 and CRS_SCAN_W1=0 in a child each -- and one launch of
         each timed shape below.  SHA-256 of the scores and ids every launch returned; equal digests are reported as 0 differing
         bytes, a differing launch is named and the status is 1.
time     A and B alternate for --rounds rounds.  A round times --launches launches of crs_cosine_topk per shape between device
         events, after a warm-up.  Shapes (the benchmark's own: overheads dominate toy sizes): 10 M x 384 fp16, 64 queries, k = 24
         (scan_tb chain, ticketed, nt); 10 M x 768 int8, 64 queries, k = 16 (scan_i8); 1.25 M x 384 fp16, 256 queries, k = 24
         (scan_wide16_kernel<384,8,24>, deferred); 100 k x 384 fp16, 64 queries, k = 10 (the dump form).  The plan the library
         describes for each shape is printed with it.  Verdict per shape: median(B) <= median(A) (1 + s), s = (max - min) / median
         of A's own rounds.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "compressed-rag-suite_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

F16, I8 = 0, 1
# (name, rows, dim, slab type, queries, k)
SHAPES = (("10M x 384 f16, 64 q, k=24", 10_000_000, 384, F16, 64, 24),
          ("10M x 768 i8, 64 q, k=16", 10_000_000, 768, I8, 64, 16),
          ("1.25M x 384 f16, 256 q, k=24", 1_250_000, 384, F16, 256, 24),
          ("100k x 384 f16, 64 q, k=10", 100_000, 384, F16, 64, 10))
FORM_PROCESSES = ("default", "CRS_SCAN_TB=0", "CRS_SCAN_WIDE=0", "CRS_SCAN_W1=0")


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(a.tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------------------------- children
def child_forms(out, process):
    """the forms of one process of tests/test_scan_forms_gpu.py, every launch's lists digested on the way to its checks"""
    import torch
    import _scan_form_cases as fc
    from rag import _native as nat
    nat.require_gpu()
    cuda = torch.device("cuda:0")
    res, search = {}, fc.search

    def recording(name, c, cuda_, k, env, id_base=0):
        sc, ids, word = search(name, c, cuda_, k, env, id_base)
        nq, n = c.full64.shape
        key = "%s k=%d nq=%d n=%d %s id_base=%d" % (name, k, nq, n, " ".join("%s=%s" % kv for kv in sorted(env.items())), id_base)
        assert key not in res, key
        res[key] = digest(sc, ids)
        print("  " + key, flush=True)
        return sc, ids, word

    fc.search = recording
    if process == "default":
        for name, case in fc.CASES.items():
            if case[5] not in fc.CHILD_LEGS:
                fc.run_form(name, cuda, fc.LEGS[case[5]])
    else:
        for name in fc.leg_names(process):
            fc.run_form(name, cuda, {})
        for name in fc.long_streams_from_elsewhere(process):
            fc.run_shape(name, fc.LONG_STREAM[name][0], fc.LONG_STREAM[name][1], cuda, {})
    json.dump(res, open(out, "w"))
    return 0


class Shape:
    """One timed shape on the device: seeded unit rows through the library's own row writer, seeded unit queries."""

    def __init__(self, rows, dim, st, nq, k, seed):
        import torch
        from rag import _native as nat
        self.nat, self.rows, self.dim, self.st, self.nq, self.k = nat, rows, dim, st, nq, k
        dev = torch.device("cuda:0")
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        self.slab = torch.zeros((rows, nat.padded_dim(dim, st)), dtype=torch.int8 if st == I8 else torch.float16, device=dev)
        self.scales = torch.zeros(rows, dtype=torch.float32, device=dev) if st == I8 else None
        for lo in range(0, rows, 250_000):
            x = torch.randn((min(250_000, rows - lo), dim), generator=g, device=dev)
            nat.slab_append_f32(x, self.slab, lo, st, scales=self.scales)
        q = torch.nn.functional.normalize(torch.randn((nq, dim), generator=g, device=dev), dim=1)
        self.q16 = nat.queries_to_f16(q, st)
        self.ws = torch.empty(nat.scan_workspace_bytes(nq, dim, k, rows), dtype=torch.uint8, device=dev)
        self.out_s = torch.empty((nq, k), dtype=torch.float32, device=dev)
        self.out_i = torch.empty((nq, k), dtype=torch.int64, device=dev)
        self.plan = nat.scan_plan_describe(nq, dim, k, rows, slab_type=st)
        torch.cuda.synchronize()

    def launch(self):
        return self.nat.cosine_topk(self.q16, self.slab, self.rows, self.dim, self.k, slab_type=self.st, scales=self.scales,
                                    workspace=self.ws, out_scores=self.out_s, out_ids=self.out_i)


def child_shapes(out, launches):
    """launches = 0: one launch per shape, digested; else microseconds per launch"""
    import torch
    from rag import _native as nat
    nat.require_gpu()
    res = {}
    for i, (name, rows, dim, st, nq, k) in enumerate(SHAPES):
        s = Shape(rows, dim, st, nq, k, seed=200 + i)
        if not launches:
            sc, ids = s.launch()
            torch.cuda.synchronize()
            res[name] = digest(sc.cpu().numpy(), ids.cpu().numpy())
        else:
            for _ in range(20):                                   # warm-up
                s.launch()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(launches):
                s.launch()
            t1.record()
            t1.synchronize()
            res[name] = t0.elapsed_time(t1) / launches * 1e3
        res["plan " + name] = s.plan
        del s
        torch.cuda.empty_cache()
    json.dump(res, open(out, "w"))
    return 0


# --------------------------------------------------------------------------------------------------------------------- parent
def run_child(libdir, mode, out, limit, extra, env=None):
    import _scan_form_cases as fc
    lib = os.path.join(os.path.abspath(libdir), "libcrs_hip.so")
    if not os.path.exists(lib) or not os.path.exists(os.path.join(os.path.dirname(lib), "libcrs_torch.so")):
        sys.exit(f"{libdir}: libcrs_hip.so / libcrs_torch.so not found")
    e = {k: v for k, v in os.environ.items() if not k.startswith("CRS_")}      # the knobs are the leg's, nothing inherited
    e.update(fc.LEGS.get(env, {}), CRS_LIB_PATH=lib)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", mode, out, str(extra)]
    print(f"[ab_scan] {mode} {extra} with {libdir} ...", flush=True)
    rc = subprocess.run(cmd, env=e, cwd=ROOT).returncode
    if rc:
        print(f"[ab_scan] child `{mode} {extra}` with {libdir} ended with status {rc}: stopping", flush=True)
        sys.exit(rc)
    return json.load(open(out))


def compare(a, b, tmp):
    lines, bad = [], 0
    for what in FORM_PROCESSES + ("shapes",):
        got = []
        for tag, libdir in (("a", a), ("b", b)):
            out = os.path.join(tmp, f"digest_{tag}.json")
            got.append(run_child(libdir, "shapes", out, 600, 0) if what == "shapes" else run_child(libdir, "forms", out, 900, what, env=what))
        got = [{k: v for k, v in g.items() if not k.startswith("plan ")} for g in got]
        differing = sorted(k for k in set(got[0]) | set(got[1]) if got[0].get(k) != got[1].get(k))
        bad += len(differing)
        forms = len({k.split(" k=")[0] for k in got[0]})
        lines.append("%-16s %3d %s, %4d launches: " % (what, forms, "shapes" if what == "shapes" else "forms", len(got[0])) +
                     ("0 differing bytes (scores, ids)" if not differing else "DIFFERENT: " + "; ".join(differing)))
    return lines, bad


def timing(a, b, rounds, launches, tmp):
    per = {"a": [], "b": []}
    for r in range(rounds):
        for tag, libdir in (("a", a), ("b", b)):
            per[tag].append(run_child(libdir, "shapes", os.path.join(tmp, f"time_{tag}_{r}.json"), 600, launches))
    lines = [f"A = {a}, B = {b}; {rounds} alternating rounds of {launches} launches per shape; microseconds per launch"]
    slower = 0
    for name, *_ in SHAPES:
        va, vb = [x[name] for x in per["a"]], [x[name] for x in per["b"]]
        ma, mb = statistics.median(va), statistics.median(vb)
        sa = (max(va) - min(va)) / ma
        ok = mb <= ma * (1.0 + sa)
        slower += not ok
        lines += ["%s: %s" % (name, per["b"][0]["plan " + name]),
                  "  A rounds %s  median %.2f  spread %.2f%%" % (" ".join("%.2f" % x for x in va), ma, 100 * sa),
                  "  B rounds %s  median %.2f  B / A %.4f  %s" % (" ".join("%.2f" % x for x in vb), mb, mb / ma,
                                                                "within A's spread" if ok else "SLOWER than A (1 + spread)")]
    return lines, slower


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        mode, out, extra = sys.argv[2:5]
        sys.exit(child_forms(out, extra) if mode == "forms" else child_shapes(out, int(extra)))
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("mode", choices=("compare", "time"))
    ap.add_argument("libdirs", nargs=2)
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=300)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        if args.mode == "compare":
            lines, bad = compare(*args.libdirs, tmp)
        else:
            lines, bad = timing(*args.libdirs, args.rounds, args.launches, tmp)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "a") as f:
            f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
