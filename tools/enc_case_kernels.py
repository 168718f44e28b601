"""Which kernels does each case of tests/_encoder_cases.py launch?  A test cannot see that, so the table is confirmed once:

    rocprofv3 --kernel-trace --stats -d OUT -o enc_cases --output-format csv -- python tools/enc_case_kernels.py run
    python tools/enc_case_kernels.py parse OUT/**/enc_cases_kernel_trace.csv > profiles/enc_cases_kernels.txt

`run` does one default forward per case (random weights of the case's shape: only the dispatch matters) and brackets it
with marker kernels -- tan_ opens a case, then its index as 7 bits of sin_ (1) / cos_ (0) -- so that `parse` can cut the
trace, which is ordered by start time on the one stream used, into cases."""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "compressed-rag-suite_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

BITS = 7


def run():
    import torch
    import _encoder_cases as ec
    dev = torch.device("cuda:0")
    m = torch.zeros(64, device=dev)
    for idx, case in enumerate(ec.ALL_CASES):
        enc = ec.hip_encoder(case, dev)
        ids, mask, lens = ec.case_inputs(case)
        ids_d, lens_d = torch.from_numpy(ids).to(dev), torch.from_numpy(lens).to(dev)
        enc.forward(ids_d, lens_d)           # allocates the workspace outside the bracket
        torch.cuda.synchronize()
        m.tan_()
        for b in range(BITS):
            m.sin_() if (idx >> b) & 1 else m.cos_()
        enc.forward(ids_d, lens_d)
        m.tan_()
        torch.cuda.synchronize()


def short_name(mangled):
    """_ZN3crs12_GLOBAL__N_117gemm_panel_kernelILi3ELi64EEEv... -> gemm_panel_kernel<3, 64> (integer / bool template arguments)."""
    import re
    m = re.match(r"_ZN3crs(?:12_GLOBAL__N_1)?(\d+)", mangled)
    if not m:
        return mangled.replace("void crs::(anonymous namespace)::", "").split("(")[0]
    n = int(m.group(1))
    name, rest = mangled[m.end():m.end() + n], mangled[m.end() + n:]
    args = []
    if rest.startswith("I"):
        rest = rest[1:]
        while True:
            a = re.match(r"L([ib])(n?\d+)E", rest)
            if not a:
                break
            args.append(a.group(2).replace("n", "-") if a.group(1) == "i" else ("true" if a.group(2) == "1" else "false"))
            rest = rest[a.end():]
    return name + (f"<{', '.join(args)}>" if args else "")


def parse(path):
    import _encoder_cases as ec
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows]

    def kind(n):
        for k in ("tan", "sin", "cos"):
            if f"{k}_kernel" in n or f"{k}_" in n.lower() and "elementwise" in n:
                return k
        return None

    i, found = 0, {}
    while i < len(names):
        if kind(names[i]) == "tan" and i + BITS < len(names) and all(kind(names[i + 1 + b]) in ("sin", "cos") for b in range(BITS)):
            idx = sum((kind(names[i + 1 + b]) == "sin") << b for b in range(BITS))
            j = i + 1 + BITS
            ks = []
            while kind(names[j]) != "tan":
                ks.append(names[j])
                j += 1
            found[idx] = ks
            i = j + 1
        else:
            i += 1
    print("Kernels of ONE default forward per case of tests/_encoder_cases.py on an MI355X (rocprofv3 --kernel-trace; tools/enc_case_kernels.py),")
    print("in launch order, each kernel listed once.  `why` is the branch the case is in the table for.\n")
    for idx, case in enumerate(ec.ALL_CASES):
        ks = found.get(idx)
        print(f"{case.name}  [{case.cfg.hidden} / {case.cfg.heads} heads / ffn {case.cfg.ffn} / {case.cfg.layers} layer(s), {case.batch} x {case.seq}]  why: {case.why}")
        if ks is None:
            print("    NOT FOUND IN THE TRACE")
            continue
        seen = []
        for k in ks:
            k = short_name(k)
            if k not in seen:
                seen.append(k)
        for k in seen:
            print("    " + k)


if __name__ == "__main__":
    run() if sys.argv[1] == "run" else parse(sys.argv[2])
