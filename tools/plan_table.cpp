// plan_table.cpp -- the scan planner (csrc/plan.cpp) as a stand-alone program: no HIP, no device.
//   g++ -O2 -std=c++17 -o plan_table tools/plan_table.cpp compressed-rag-suite_amd/csrc/plan.cpp
//   ./plan_table <CUs> < cases            one case per line: nq dim k n_rows slab_type (0 fp16, 1 int8)
//   ./plan_table --forms                  one line per kernel instantiation the predicates of csrc/scan_forms.h admit
//   ./plan_table --ring <CUs> < cases     per case: ring lds ticket t_dyn dyn_mask describe-text (the wide kernel's buffer scheme)
// The knobs come from the environment (CRS_SCAN_TB=0 ./plan_table 256 ...), as in the library.  One tab-separated line per case:
//   family waves slots tile_rows n_tiles streams qblocks kp nt ticket t_dyn dyn_mask boot sched no_stagger mfma form_exists
//   workspace_bytes describe-text
// (workspace_bytes is what crs_scan_workspace_bytes answers; the text is crs_scan_plan_describe's up to "; cert tail:").
// --forms spells every name as plan_describe does, wide forms with /mfma16 or /mfma32 behind (tests/test_scan_forms_cpu.py holds
// the case table of tests/_scan_form_cases.py against this list).
// tests/test_plan_cpu.py drives it; for a sanitizer run add -fsanitize=address,undefined to the g++ line.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../compressed-rag-suite_amd/csrc/plan.h"

// Every argument range is wider than what exists: the predicates, not these loops, decide.
static int list_forms() {
  using namespace crs;
  for (int d = 64; d <= 1152; d += 64) {
    for (int nw = 2; nw <= 16; nw += 2)
      for (int s = 0; s <= 72; ++s)
        if (tb_form_exists(d, nw, s)) printf("scan_tb_kernel<%d,%d,%d,%d>\n", d, tb_tile_rows(d), nw, s);
    for (int nw = 2; nw <= 16; nw += 2)
      for (int s = 0; s <= 72; ++s)
        for (int mfma = 16; mfma <= 32; mfma += 16)
          if (wide_form_exists(d, nw, s, mfma)) printf("scan_wide_kernel<%d,%d,%d>/mfma%d\n", d, nw, s, mfma);
    for (int s = 0; s <= 72; ++s)
      if (i8_form_exists(d, s)) printf("scan_i8_kernel<%d,%d,16,%d>\n", d, i8_tile_rows(), s);
    for (int l = 8; l <= 64; l += 8) {   // the threshold kernels: L is classic_list_slots(k)
      if (l != classic_list_slots(l)) continue;
      if (i8_form_exists(d, -1)) printf("scan_i8_kernel<%d,%d,%d,-1>\n", d, i8_tile_rows(), l);
      if (classic_form_exists(d, l)) printf("scan_f16_kernel<%d,%d,%d>\n", d, classic_tile_rows(d), l);
    }
    if (w1_form_exists(d)) printf("scan_w2_kernel<%d>\n", d);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--forms")) return list_forms();
  const bool ring_cols = argc == 3 && !strcmp(argv[1], "--ring");
  if (ring_cols) { --argc; ++argv; }
  if (argc != 2 || atoi(argv[1]) <= 0) { fprintf(stderr, "usage: plan_table [--ring] <CUs> < cases | plan_table --forms\n"); return 2; }
  const int cus = atoi(argv[1]);
  static const char* const kFamily[] = {"Classic", "TileBest", "Wide", "W1"};
  int nq, dim, k, slab_type;
  long long n_rows;
  while (scanf("%d %d %d %lld %d", &nq, &dim, &k, &n_rows, &slab_type) == 5) {
    const crs::Knobs kn = crs::knobs_from_env();
    crs::Plan p;
    const char* why = "";
    size_t ws = 0;
    char text[192];
    if (crs::make_plan(nq, dim, k, n_rows, slab_type, cus, kn, &p, &why) || crs::plan_workspace_bytes(nq, dim, k, n_rows, cus, kn, &ws, &why)) {
      printf("error\t%s\n", why);
      continue;
    }
    crs::plan_describe(p, text, sizeof text);
    if (ring_cols) {
      printf("%d\t%d\t%d\t%d\t%d\t%s\n", (int)p.ring, p.lds, (int)p.ticket, p.t_dyn, p.dyn_mask, text);
      continue;
    }
    printf("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%zu\t%s\n", kFamily[(int)p.family], p.waves, p.slots, p.tile_rows,
           p.n_tiles, p.nwg, p.nqb, p.kp, p.nt, (int)p.ticket, p.t_dyn, p.dyn_mask, p.boot, p.sched, p.no_stagger, p.mfma, (int)p.form_exists(),
           ws, text);
  }
  return 0;
}
