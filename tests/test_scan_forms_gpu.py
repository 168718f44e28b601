"""On the device: every scan kernel instantiation the planner can pick runs once against an fp64 product of the same numbers.

tests/_scan_form_cases.py holds one case per form (166; tests/test_scan_forms_cpu.py proves the table closed over
csrc/scan_forms.h) and everything a run does: assert the describe text, poison the workspace, launch crs_cosine_topk, run
topk_check.check_topk (TIGHT_TOL and BAND as they are) over all queries, demand the exact fp64 order -- ties by id, duplicate
scores bit-equal -- on the planted queries; then the form's smallest k (dump and threshold forms), the ticketed tile schedule
against the static one bit for bit (chain forms whose plan allows it), id_base = 2^40 + 5 (one form per family), and the second
shapes: above the bootstrap (threshold forms that have one), two query blocks (8-wave wide forms), and for the scan_tb / scan_i8
chain forms whose case leaves slots empty a stream longer than the chain has slots, under whichever leg reaches it.

The default-knob forms and both MFMA shapes of the dual-shape wide forms run in this process (CRS_WIDE_MFMA is re-read per call).
CRS_SCAN_TB=0, CRS_SCAN_WIDE=0 and CRS_SCAN_W1=0 are read once per process: each of those legs runs its forms in one fresh child,
one child after another, each under its own timeout; then one child per staging variant CRS_SCAN_VARIANT = 0, 1, 2 of scan.hip
runs the 16 fp16 threshold forms.  A child stops at its first failed form; one that ends abnormally fails its test and no
further child is started.  Measured score ratios: profiles/scan_forms_ratios.txt, which test_zz_score_ratios writes to the path
CRS_SCAN_FORMS_RATIOS names."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _scan_form_cases as fc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN_PROCESS = [n for n, c in fc.CASES.items() if c[5] not in fc.CHILD_LEGS]
DUAL_SHAPE = [n[:-len("/mfma16")] for n in fc.CASES if n.endswith("/mfma16")]
_RAN = {"abnormal": None}


@pytest.mark.parametrize("name", IN_PROCESS)
def test_form(cuda, name):
    assert "CRS_WIDE_MFMA" not in os.environ and not any(v in os.environ for leg in fc.CHILD_LEGS for v in fc.LEGS[leg])
    fc.run_form(name, cuda, fc.LEGS[fc.CASES[name][5]])


@pytest.mark.parametrize("form", DUAL_SHAPE)
def test_both_mfma_shapes_return_one_list(cuda, form):
    """the forms that exist on 32x32x16 and on 16x16x32 MFMAs: the same corpus through both, equal final lists"""
    a, b = form + "/mfma16", form + "/mfma32"
    assert fc.CASES[a][:5] == fc.CASES[b][:5]
    nq, _, k, n = fc.CASES[a][:4]
    streams = fc.plan_of(a, nq, n, k, {"CRS_WIDE_MFMA": "16"})[0]
    assert streams == fc.plan_of(b, nq, n, k, {"CRS_WIDE_MFMA": "32"})[0]
    c = fc.corpus_of(a, nq, n, streams)
    s16, i16, _ = fc.search(a, c, cuda, k, {"CRS_WIDE_MFMA": "16"})
    s32, i32, _ = fc.search(b, c, cuda, k, {"CRS_WIDE_MFMA": "32"})
    assert np.array_equal(i16, i32) and np.array_equal(s16.view(np.int32), s32.view(np.int32))


def _child(env, args, names, what):
    """One fresh process for the forms `names`; fails on anything but "every form ran and passed"."""
    if _RAN["abnormal"]:
        pytest.fail("not started: the child for %s ended abnormally" % _RAN["abnormal"])
    e = {k: v for k, v in os.environ.items() if not k.startswith("CRS_")}
    e.update(env)
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_scan_form_cases.py")] + args, cwd=ROOT, env=e,
                           capture_output=True, text=True, timeout=900)
    except subprocess.TimeoutExpired:
        _RAN["abnormal"] = what
        raise
    lines = r.stdout.splitlines()
    if r.returncode not in (0, 1):
        _RAN["abnormal"] = what
        pytest.fail("%s: the child ended with status %d\n%s\n%s" % (what, r.returncode, r.stdout[-3000:], r.stderr[-3000:]))
    print("\n".join(l for l in lines if l.startswith(("RATIO", "FAIL"))))
    for l in lines:
        if l.startswith("RATIO "):
            fam, x = l.split()[1:]
            fc.RATIOS[fam] = max(fc.RATIOS.get(fam, 0.0), float(x))
        if l.startswith("CASE "):
            fc.CASE_RATIOS.append((float(l.split()[1]), l.split(" ", 2)[2] + " (" + what + ")"))
    failed = [l for l in lines if l.startswith("FAIL ")]
    assert not failed and r.returncode == 0, "%s: %s\n%s" % (what, failed[:5], r.stderr[-2000:])
    assert [l[5:] for l in lines if l.startswith("PASS ")] == names, what      # every form of the leg, none filtered out, in order


def test_static_knob_legs_in_child_processes(cuda):
    ran = 0
    for leg in fc.CHILD_LEGS:
        names = fc.leg_names(leg)
        # then the long-stream shapes that need this leg's knobs, of forms whose own case runs elsewhere
        _child(fc.LEGS[leg], [leg], names + ["long " + n for n in fc.long_streams_from_elsewhere(leg)], leg)
        ran += len(names)
    assert ran + len(IN_PROCESS) == len(fc.CASES) == 166
    assert not fc.long_streams_from_elsewhere("default")      # test_form runs every other long-stream shape


def test_classic_staging_variants_in_child_processes(cuda):
    """scan.hip's staging variants 0 (register-staged), 1 (LDS-DMA ring, one workgroup per CU) and 2 (LDS-DMA double buffer):
    selectable in production by CRS_SCAN_VARIANT, the default is 3."""
    names = [n for n in fc.leg_names("CRS_SCAN_TB=0") if fc.family(n) == "scan_f16"]
    assert len(names) == 16
    for variant in "012":
        _child(dict(fc.LEGS["CRS_SCAN_TB=0"], CRS_SCAN_VARIANT=variant), ["CRS_SCAN_TB=0", "f16-classic"], names,
               "CRS_SCAN_VARIANT=" + variant)


def test_zz_score_ratios(cuda):
    """The worst |score - fp64| / TIGHT_TOL per kernel family over everything this module ran (children included), and the ten
    largest single launches.  CRS_SCAN_FORMS_RATIOS names a file to write them to: the body of profiles/scan_forms_ratios.txt."""
    from topk_check import TIGHT_TOL
    lines = ["%d checked launches; worst max |score - fp64| / TIGHT_TOL per kernel family:" % len(fc.CASE_RATIOS), ""]
    lines += ["%s %.3f" % (fam, r) for fam, r in sorted(fc.RATIOS.items())]
    lines += ["", "the ten largest launches:", ""] + ["%.3f %s" % x for x in sorted(fc.CASE_RATIOS, reverse=True)[:10]]
    print("TIGHT_TOL = %g\n%s" % (TIGHT_TOL, "\n".join(lines)))
    assert all(r <= 1.0 for r in fc.RATIOS.values())
    out = os.environ.get("CRS_SCAN_FORMS_RATIOS")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
