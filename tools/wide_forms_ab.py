#!/usr/bin/env python3
"""Time the forms of csrc/scan_wide.hip, scan kernel alone (crs_time_cosine_topk's second figure), one JSON line per form.

  python tools/wide_forms_ab.py [--knob CRS_WIDE_DEFER] [--rounds 5] [--iters 20] [--rows 2000000] [--tag NAME] FORM ...
  FORM = dim,queries,k   e.g. 384,256,32 (scan_wide_kernel<384,8,32>), 256,256,24, 384,128,10 (the 4-wave kernel)

With --knob the environment variable is alternated 1 / 0 inside the process, round by round (the knobs of plan.h marked "per call"
are read at every plan); without it the library is timed as built, and a job alternates builds by running this once per tree.
Rows are seeded unit rows that do not repeat -- the deferred insertion's work depends on the data.  Each line: the form, the plan,
and per arm the ms of every round, their median and spread."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "compressed-rag-suite_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("forms", nargs="+")
    ap.add_argument("--knob", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    import torch
    from rag import _native as nat
    nat.require_gpu()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(14)
    slabs = {}
    for form in args.forms:
        dim, nq, k = (int(x) for x in form.split(","))
        if dim not in slabs:
            slabs.clear()
            torch.cuda.empty_cache()
            rows = torch.nn.functional.normalize(torch.randn((args.rows, dim), generator=g, device=dev), dim=1)
            slabs[dim] = rows.to(torch.float16).contiguous()
        slab = slabs[dim]
        q16 = torch.nn.functional.normalize(torch.randn((nq, dim), generator=g, device=dev), dim=1).to(torch.float16).contiguous()
        arms = {"1": [], "0": []} if args.knob else {"built": []}
        nat.time_cosine_topk(q16, slab, args.rows, dim, k, 3)      # warm-up
        for _ in range(args.rounds):
            for arm in arms:
                if args.knob:
                    os.environ[args.knob] = arm
                arms[arm].append(round(nat.time_cosine_topk(q16, slab, args.rows, dim, k, args.iters)[1], 5))
        if args.knob:
            os.environ.pop(args.knob, None)
        out = {"form": form, "tag": args.tag, "knob": args.knob, "rows": args.rows, "iters": args.iters,
               "plan": nat.scan_plan_describe(nq, dim, k, args.rows)}
        for arm, ms in arms.items():
            out[f"ms_{arm}"] = ms
            out[f"median_{arm}"] = statistics.median(ms)
            out[f"spread_{arm}"] = round(max(ms) - min(ms), 5)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
