#!/usr/bin/env python3
"""A/B of the row writers (csrc/row_build.hip, csrc/slab_row.h) between two builds of the libraries: same bits, same speed.

  python tools/ab_row_build.py record  LIBDIR           [--out tests/golden/row_build_bits.npz]
  python tools/ab_row_build.py compare LIBDIR_A LIBDIR_B
  python tools/ab_row_build.py time    LIBDIR_A LIBDIR_B [--rounds 5] [--launches 1000] [--out profiles/row_build_ab.txt]

A LIBDIR holds libcrs_hip.so and libcrs_torch.so of one build.  Every measurement runs in a fresh child process that loads that
build through CRS_LIB_PATH, one child at a time (so never more than two processes hold the GPU: this one does not open it), each
under its own `timeout`; the first child that ends with a non-zero status ends the run with that status.

record   the cases of tests/_row_bits.py through LIBDIR -> the fixture of tests/test_row_build_bits_gpu.py (inputs and what the
         library wrote).  Record with the build whose bits are to be kept.
compare  both builds on the same seeded inputs at the sizes of `time`: SHA-256 of every array a job wrote (slab, scales, shadow,
         row error).  Equal digests are reported as 0 differing bytes; a differing array is named and the status is 1.
time     A and B alternate for --rounds rounds.  A round times --launches launches per size between device events, after a warm-up,
         in segments of 100 launches (the rescale restores its shadow between segments, outside the events: 100 halvings keep
         fp32 values normal).  Sizes: one build step of the benchmark's stores (245 760 rows), an update of 65 536 rows of a store
         of 1 M rows, a rescale of 1 M rows.  Verdict per size: median(B) <= median(A) (1 + s), s = (max - min) / median of A's own
         rounds.
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

BUILD_ROWS = 245760
STORE_ROWS = 1 << 20
UPDATE_ROWS = 65536
SEGMENT = 100
# (name, space, slab type, dim, job)
SIZES = (("append cosine f16 245760x384", "cosine", 0, 384, "append"),
         ("append cosine i8 245760x768", "cosine", 1, 768, "append"),
         ("append ip f16 245760x384", "ip", 0, 384, "append"),
         ("append l2 f16 245760x384", "l2", 0, 384, "append"),
         ("scatter cosine f16 65536 of 1Mx384", "cosine", 0, 384, "scatter"),
         ("rescale l2 f16 1Mx384", "l2", 0, 384, "rescale"))


# ------------------------------------------------------------------------------------------------------------------- children
class Job:
    """One size on the device: seeded inputs, zeroed arrays, launch()."""

    def __init__(self, space, st, dim, job, seed):
        import torch
        from rag import _native as nat
        self.nat, self.torch, self.job, self.st, self.dim = nat, torch, job, st, dim
        self.space = nat.SPACES[space]
        dev = torch.device("cuda:0")
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        self.rows = STORE_ROWS if job != "append" else BUILD_ROWS
        m = {"append": BUILD_ROWS, "scatter": UPDATE_ROWS, "rescale": STORE_ROWS}[job]
        # norms spread around 1 (all below R = 4), a zero row and a tiny row among them
        self.emb = torch.randn((m, dim), generator=g, device=dev) * (torch.rand((m, 1), generator=g, device=dev) + 0.5) / dim ** 0.5
        self.emb[1] = 0.0
        self.emb[2] *= 1e-15
        sdim = nat.space_row_dim(dim, self.space)
        self.slab = torch.zeros((self.rows, nat.padded_dim(sdim, st)), dtype=torch.int8 if st == nat.SLAB_I8 else torch.float16, device=dev)
        self.scales = torch.zeros(self.rows, dtype=torch.float32, device=dev) if st == nat.SLAB_I8 else None
        self.shadow = torch.zeros((self.rows, sdim), dtype=torch.float32, device=dev)
        self.row_err = torch.zeros(1, dtype=torch.float32, device=dev)
        self.norm_scale = torch.full((1,), 4.0, dtype=torch.float32, device=dev)
        self.kw = dict(scales=self.scales, shadow=self.shadow, row_err=self.row_err)
        self.local = torch.randperm(STORE_ROWS, generator=g, device=dev)[:UPDATE_ROWS].contiguous() if job == "scatter" else None
        self.shadow0 = None
        if job == "rescale":                    # the rows to rescale: an append under R = 4
            nat.slab_append_space_f32(self.emb, self.space, self.norm_scale, self.slab, 0, **self.kw)
            self.shadow0 = self.shadow.clone()
        torch.cuda.synchronize()

    def restore(self):
        if self.shadow0 is not None:
            self.shadow.copy_(self.shadow0)

    def launch(self):
        nat = self.nat
        if self.job == "rescale":
            nat.slab_rescale_space(self.rows, self.dim, self.space, 1, self.slab, self.shadow, scales=self.scales, row_err=self.row_err)
        elif self.space == nat.SPACE_COSINE and self.job == "append":
            nat.slab_append_f32(self.emb, self.slab, 0, self.st, **self.kw)
        elif self.space == nat.SPACE_COSINE:
            nat.slab_write_rows_f32(self.emb, self.local, self.slab, self.rows, **self.kw)
        elif self.job == "append":
            nat.slab_append_space_f32(self.emb, self.space, self.norm_scale, self.slab, 0, **self.kw)
        else:
            nat.slab_write_rows_space_f32(self.emb, self.local, self.space, self.norm_scale, self.slab, self.rows, **self.kw)

    def digests(self):
        out = {}
        for name, t in (("slab", self.slab), ("scales", self.scales), ("shadow", self.shadow), ("row_err", self.row_err)):
            if t is not None:
                h = hashlib.sha256()
                flat = t.view(self.torch.int16 if t.dtype == self.torch.float16 else t.dtype).reshape(-1)
                for lo in range(0, flat.numel(), 1 << 26):
                    h.update(flat[lo: lo + (1 << 26)].cpu().numpy().tobytes())
                out[name] = h.hexdigest()
        return out


def child_record(out):
    import numpy as np
    import torch
    import _row_bits as rb
    from rag import _native as nat
    nat.require_gpu()
    dev = torch.device("cuda:0")
    arrays = {}
    for kind, st, dim, R in rb.CASES:
        x = arrays.setdefault(rb.input_key(kind, dim, R), rb.make_input(kind, dim, R))
        for name, arr in rb.run_case(kind, st, dim, R, x, dev).items():
            arrays[rb.key(kind, st, dim, R) + "/" + name] = arr
    np.savez_compressed(out, **arrays)
    size = os.path.getsize(out)
    print(f"recorded {len(rb.CASES)} cases, {len(arrays)} arrays, {size} bytes -> {out}")
    return 0 if size < 512 * 1024 else 1


def child_digest(out):
    import torch
    from rag import _native as nat
    nat.require_gpu()
    res = {}
    for i, (name, space, st, dim, job) in enumerate(SIZES):
        j = Job(space, st, dim, job, seed=100 + i)
        j.launch()
        torch.cuda.synchronize()
        res[name] = j.digests()
        del j
        torch.cuda.empty_cache()
    json.dump(res, open(out, "w"))
    return 0


def child_time(out, launches):
    import torch
    from rag import _native as nat
    nat.require_gpu()
    res = {}
    for i, (name, space, st, dim, job) in enumerate(SIZES):
        j = Job(space, st, dim, job, seed=100 + i)
        for _ in range(10):                                   # warm-up
            j.launch()
        total = 0.0
        for lo in range(0, launches, SEGMENT):
            j.restore()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(min(SEGMENT, launches - lo)):
                j.launch()
            t1.record()
            t1.synchronize()
            total += t0.elapsed_time(t1)
        res[name] = total / launches * 1e3                    # microseconds per launch
        del j
        torch.cuda.empty_cache()
    json.dump(res, open(out, "w"))
    return 0


# --------------------------------------------------------------------------------------------------------------------- parent
def run_child(libdir, mode, out, limit, *extra):
    lib = os.path.join(os.path.abspath(libdir), "libcrs_hip.so")
    if not os.path.exists(lib) or not os.path.exists(os.path.join(os.path.dirname(lib), "libcrs_torch.so")):
        sys.exit(f"{libdir}: libcrs_hip.so / libcrs_torch.so not found")
    env = dict(os.environ, CRS_LIB_PATH=lib)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", mode, out, *extra]
    print(f"[ab_row_build] {mode} with {libdir} ...", flush=True)
    rc = subprocess.run(cmd, env=env, cwd=ROOT).returncode
    if rc:
        print(f"[ab_row_build] child `{mode}` with {libdir} ended with status {rc}: stopping", flush=True)
        sys.exit(rc)


def compare(a, b, tmp):
    got = []
    for tag, libdir in (("a", a), ("b", b)):
        out = os.path.join(tmp, f"digest_{tag}.json")
        run_child(libdir, "digest", out, 600)
        got.append(json.load(open(out)))
    lines, bad = [], 0
    for name in got[0]:
        differing = [arr for arr in got[0][name] if got[0][name][arr] != got[1][name].get(arr)]
        bad += len(differing)
        lines.append(f"{name}: " + ("0 differing bytes (%s)" % ", ".join(got[0][name]) if not differing else "DIFFERENT: " + ", ".join(differing)))
    return lines, bad


def timing(a, b, rounds, launches, tmp):
    per = {"a": [], "b": []}
    for r in range(rounds):
        for tag, libdir in (("a", a), ("b", b)):
            out = os.path.join(tmp, f"time_{tag}_{r}.json")
            run_child(libdir, "time", out, 900, str(launches))
            per[tag].append(json.load(open(out)))
    lines = [f"A = {a}, B = {b}; {rounds} alternating rounds of {launches} launches per size; microseconds per launch",
             "%-40s %10s %8s %10s %8s %8s  %s" % ("size", "A median", "A spread", "B median", "B spread", "B / A", "verdict")]
    slower = 0
    for name, *_ in SIZES:
        va, vb = [x[name] for x in per["a"]], [x[name] for x in per["b"]]
        ma, mb = statistics.median(va), statistics.median(vb)
        sa, sb = (max(va) - min(va)) / ma, (max(vb) - min(vb)) / mb
        ok = mb <= ma * (1.0 + sa)
        slower += not ok
        lines.append("%-40s %10.2f %7.2f%% %10.2f %7.2f%% %8.4f  %s" % (name, ma, 100 * sa, mb, 100 * sb, mb / ma,
                                                                      "within A's spread" if ok else "SLOWER than A (1 + spread)"))
    return lines, slower


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        mode, out, extra = sys.argv[2], sys.argv[3], sys.argv[4:]
        sys.exit({"record": child_record, "digest": child_digest}[mode](out) if mode != "time" else child_time(out, int(extra[0])))
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("mode", choices=("record", "compare", "time"))
    ap.add_argument("libdirs", nargs="+")
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=1000)
    args = ap.parse_args()
    if len(args.libdirs) != (1 if args.mode == "record" else 2):
        ap.error("record takes one LIBDIR, compare and time take two")
    if args.mode == "record":
        out = os.path.abspath(args.out or os.path.join(ROOT, "tests", "golden", "row_build_bits.npz"))
        run_child(args.libdirs[0], "record", out, 300)
        return 0
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
