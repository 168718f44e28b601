// mxfp4_plan.cpp -- the plan of an MXFP4 sweep (mxfp4.h): plain C++17, no HIP, runs without a device.
#include "mxfp4.h"

#include <stdio.h>

namespace crs {

static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

int mx_make_plan(int nq, int dim, int kp, int64_t n_rows, int cus, MxPlan* p, const char** why) {
  if (nq < 1 || nq > kMxMaxQ) { *why = "nq must be in 1..64 (larger batches run as more sweeps)"; return -1; }
  if (dim < 1 || dim > 1024) { *why = "dim must be in 1..1024"; return -1; }
  if (kp != 32 && kp != 64 && kp != 128) { *why = "kp must be 32, 64 or 128"; return -1; }
  if (n_rows < 1 || n_rows >= ((int64_t)1 << 31) - 64) { *why = "n_rows must be in 1..2^31 - 65"; return -1; }
  if (cus < 1) cus = 256;
  p->nq = nq;
  p->kp = kp;
  p->pdim = mx_pdim(dim);
  p->ksteps = p->pdim / 128;
  p->groups = (nq + 15) / 16;
  p->n_tiles = mx_tiles(n_rows);
  // one workgroup per CU: its waves (one per query group) share every tile they load, and a stream shorter than 4 tiles would
  // spend its time on the list flush
  int64_t nwg = p->n_tiles / 4;
  if (nwg > cus) nwg = cus;
  if (nwg < 1) nwg = 1;
  p->nwg = (int)nwg;
  p->cap = 2 * kp;
  p->lds = p->groups * 16 * p->cap * 8;
  p->levels = p->nwg > kMxMergeFan ? 2 : 1;
  p->q_bytes = (size_t)p->groups * p->ksteps * 64 * 32;
  p->qs_bytes = (size_t)p->groups * 64 * 8;
  p->part_elems = (size_t)p->nwg * nq * kp;
  p->inter_elems = p->levels == 2 ? (size_t)((p->nwg + kMxMergeFan - 1) / kMxMergeFan) * nq * kp : 0;
  return 0;
}

int mx_plan_describe(const MxPlan& p, char* buf, size_t cap) {
  return snprintf(buf, cap, "scan_mxfp4<ksteps=%d,kp=%d> streams=%d waves=%d lds=%d + merge_sorted x%d", p.ksteps, p.kp, p.nwg,
                  p.groups, p.lds, p.levels);
}

MxWs mx_ws_layout(const MxPlan& p) {
  MxWs w;
  size_t at = 0;
  w.q = at; at += up256(p.q_bytes);
  w.qs = at; at += up256(p.qs_bytes);
  w.part_s = at; at += up256(p.part_elems * 4);
  w.part_i = at; at += up256(p.part_elems * 8);
  w.inter_s = at; at += up256(p.inter_elems * 4);
  w.inter_i = at; at += up256(p.inter_elems * 8);
  w.bytes = at;
  return w;
}

}  // namespace crs
