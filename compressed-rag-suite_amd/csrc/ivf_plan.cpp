// ivf_plan.cpp -- the plan of an IVF probe (ivf.h): plain C++17, no HIP, runs without a device.
#include "ivf.h"

#include <stdio.h>

#include "scan_forms.h"

namespace crs {

static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

int ivf_make_plan(int nq, int dim, int nprobe, int k, int kp, int64_t n_rows, int64_t nlist, IvfPlan* p, const char** why) {
  if (nq < 1 || nq > kIvfMaxQ) { *why = "nq must be in 1..256 (larger batches run as more calls)"; return -1; }
  if (nprobe < 1 || nprobe > kIvfMaxProbe) { *why = "nprobe must be in 1..64"; return -1; }
  if (nlist < 1 || nlist > kIvfMaxLists) { *why = "nlist must be in 1..2^18"; return -1; }
  if (dim < 1 || dim > 1024) { *why = "dim must be in 1..1024"; return -1; }
  if (kp != 32 && kp != 64) { *why = "kp must be 32 or 64"; return -1; }
  if (k < 1 || k > kp) { *why = "k must be in 1..kp"; return -1; }
  if (n_rows < 1 || n_rows >= ((int64_t)1 << 31)) { *why = "n_rows must be in 1..2^31 - 1"; return -1; }
  p->nq = nq;
  p->nprobe = nprobe;
  p->kp = kp;
  p->k = k;
  p->pdim = row_elems(dim, kSlabF16);
  p->ksteps = p->pdim / 32;
  p->pairs = nq * nprobe;
  int n = 64;
  while (n < p->pairs) n <<= 1;
  p->sort_n = n;
  p->group_threads = n < 1024 ? n : 1024;
  p->group_lds = n * 4 + p->group_threads * 4;
  // Four waves, one per SIMD: a wave then owns up to 512 registers, which the 1024-element row needs (128 for the queries, 128
  // per tile in flight).  Short rows leave room for a deeper ring.
  p->waves = kIvfWaves;
  p->ring = p->ksteps <= 8 ? 4 : 2;
  p->cap = 2 * kp;
  p->probe_lds = p->waves * kIvfItemPairs * p->cap * 8;
  return 0;
}

int ivf_plan_describe(const IvfPlan& p, char* buf, size_t cap) {
  return snprintf(buf, cap, "ivf_group<n=%d,threads=%d> lds=%d + ivf_probe<ksteps=%d,kp=%d> grid<=%d waves=%d ring=%d lds=%d + merge x1",
                  p.sort_n, p.group_threads, p.group_lds, p.ksteps, p.kp, p.pairs, p.waves, p.ring, p.probe_lds);
}

IvfWs ivf_ws_layout(const IvfPlan& p) {
  IvfWs w;
  size_t at = 0;
  w.header = at; at += 256;
  w.keys = at; at += up256((size_t)p.pairs * 4);
  w.items = at; at += up256((size_t)p.pairs * 4);
  w.part_s = at; at += up256((size_t)p.pairs * p.kp * 4);
  w.part_r = at; at += up256((size_t)p.pairs * p.kp * 4);
  w.bytes = at;
  return w;
}

}  // namespace crs
