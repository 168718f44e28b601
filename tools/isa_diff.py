#!/usr/bin/env python3
"""Per-kernel resources and instruction mix of two source trees, side by side: the compiler evidence of a refactor.

  python tools/isa_diff.py PARENT_CSRC NEW_CSRC [file.hip ...]        (default: every *.hip both trees have; exit 1 on a violation)

Each translation unit of both trees is compiled for gfx950 to assembly with tools/check_resources.py's flags.  Per kernel, from the
kernel metadata: VGPRs (AGPRs included), SGPRs, scratch bytes per lane, static LDS bytes; from the kernel's body, instructions
counted by the class its mnemonic's prefix names:
  mfma     v_mfma* v_smfmac*            lds      ds_*               vmem   global_* buffer_* flat_* scratch_*
  valu     any other v_*                waitcnt  s_waitcnt*         barrier s_barrier*          salu   any other s_*
One line per kernel: the new tree's figures, and "parent -> new" wherever the two differ.  Violations:
  * the two trees' kernel symbols differ;
  * scratch differs (zero stays zero; a kernel that already spills may not spill more);
  * VGPRs above the parent's;
  * the mfma, lds, vmem, waitcnt or barrier count differs.
A different valu count is no violation; the kernels are grouped by WHICH v_* mnemonics changed by how much, one line per distinct
pattern, for the reader to put a cause to.
"""
import collections
import concurrent.futures as cf
import glob
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_resources import FLAGS, HIPCC, demangle  # noqa: E402

CLASSES = ("mfma", "lds", "vmem", "valu", "waitcnt", "barrier", "salu")
PINNED = ("mfma", "lds", "vmem", "waitcnt", "barrier")


def klass(mn):
    if mn.startswith(("v_mfma", "v_smfmac")):
        return "mfma"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if mn.startswith("s_waitcnt"):
        return "waitcnt"
    if mn.startswith("s_barrier"):
        return "barrier"
    return "valu" if mn.startswith("v_") else "salu" if mn.startswith("s_") else None


def kernels_of(path):
    """{symbol: (meta dict, Counter by class, Counter of v_* mnemonics)} of one translation unit"""
    r = subprocess.run([HIPCC, *FLAGS, "-S", path, "-o", "-"], capture_output=True, text=True, cwd=os.path.dirname(path))
    if r.returncode:
        sys.exit("%s does not compile:\n%s" % (path, r.stderr[-2000:]))
    s = r.stdout
    meta = {}
    for block in re.split(r"^  - (?=\.)", s[s.find("amdhsa.kernels:"):], flags=re.M)[1:]:
        f = dict(re.findall(r"^ {0,4}(\.\w+):\s+(\S+)$", "    " + block, flags=re.M))
        if ".symbol" in f:
            meta[f[".name"]] = {"vgpr": int(f[".vgpr_count"]), "sgpr": int(f[".sgpr_count"]),
                                "scratch": int(f[".private_segment_fixed_size"]), "lds": int(f[".group_segment_fixed_size"])}
    out = {}
    for name, m in meta.items():
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(name), s, flags=re.S | re.M).group(1)
        by_class, valu = collections.Counter(), collections.Counter()
        for ln in body.splitlines():
            mn = re.match(r"\s+([a-z]\w+)", ln)
            c = klass(mn.group(1)) if mn else None
            if c:
                by_class[c] += 1
                if c == "valu":
                    valu[mn.group(1)] += 1
        out[name] = (m, by_class, valu)
    return out


def show(a, b):
    return "%d" % b if a == b else "%d->%d" % (a, b)


def main(argv):
    if len(argv) < 2:
        sys.exit(__doc__)
    parent, new = (os.path.abspath(p) for p in argv[:2])
    files = argv[2:] or sorted(set(map(os.path.basename, glob.glob(os.path.join(parent, "*.hip")))) &
                               set(map(os.path.basename, glob.glob(os.path.join(new, "*.hip")))))
    jobs = [os.path.join(tree, f) for f in files for tree in (parent, new)]
    with cf.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        got = dict(zip(jobs, ex.map(kernels_of, jobs)))
    bad, total, lower, equal, spilling = [], 0, 0, 0, 0
    patterns = collections.defaultdict(list)
    print("%-96s %9s %9s %9s %7s | %s   (total)" % ("kernel", "VGPRs", "SGPRs", "scratch", "LDS", "  ".join(CLASSES)))
    for f in files:
        a, b = got[os.path.join(parent, f)], got[os.path.join(new, f)]
        if set(a) != set(b):
            bad.append("%s: kernel symbols differ: only in parent %s, only in new %s" % (f, sorted(set(a) - set(b))[:4], sorted(set(b) - set(a))[:4]))
        syms = sorted(set(a) & set(b))
        for sym, nice in zip(syms, demangle(syms)):
            (ma, ca, va), (mb, cb, vb) = a[sym], b[sym]
            nice = nice.replace("crs::(anonymous namespace)::", "").replace("void ", "").replace("(crs::ScanArgs)", "")
            total += 1
            lower += mb["vgpr"] < ma["vgpr"]
            equal += mb["vgpr"] == ma["vgpr"]
            spilling += mb["scratch"] > 0
            print("%-96s %9s %9s %9s %7s | %s   (%s)" % (
                (f[:-4] + ": " + nice)[:96], show(ma["vgpr"], mb["vgpr"]), show(ma["sgpr"], mb["sgpr"]), show(ma["scratch"], mb["scratch"]),
                show(ma["lds"], mb["lds"]), "  ".join("%s %s" % (c, show(ca[c], cb[c])) for c in CLASSES),
                show(sum(ca.values()), sum(cb.values()))))
            if mb["scratch"] != ma["scratch"]:
                bad.append("%s: scratch %d -> %d bytes per lane" % (nice, ma["scratch"], mb["scratch"]))
            if mb["vgpr"] > ma["vgpr"]:
                bad.append("%s: VGPRs %d -> %d" % (nice, ma["vgpr"], mb["vgpr"]))
            for c in PINNED:
                if ca[c] != cb[c]:
                    bad.append("%s: %s instructions %d -> %d" % (nice, c, ca[c], cb[c]))
            if va != vb:
                delta = ", ".join("%s %+d" % (m, vb[m] - va[m]) for m in sorted(set(va) | set(vb)) if va[m] != vb[m])
                patterns["net %+d: %s" % (cb["valu"] - ca["valu"], delta)].append(nice)
    print("\n%d kernels in %d files: VGPRs equal in %d, lower in %d, higher in %d; %d kernels use scratch (as in the parent unless named "
          "below); %d violation(s)" % (total, len(files), equal, lower, total - equal - lower, spilling, len(bad)))
    print("\nvector-ALU differences, one line per distinct pattern (%d kernels differ):" % sum(map(len, patterns.values())))
    for pat, names in sorted(patterns.items(), key=lambda kv: -len(kv[1])):
        print("  %3d kernels  %s   e.g. %s" % (len(names), pat, names[0]))
    for v in bad:
        print("  VIOLATION", v)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
