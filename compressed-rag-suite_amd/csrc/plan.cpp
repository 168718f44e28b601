// plan.cpp -- the planner of a search's scan (plan.h).  Plain C++17: builds into libcrs_hip.so and alone with g++.
#include "plan.h"

#include <assert.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/crs_hip.h"

namespace crs {
namespace {

bool env_on(const char* name) {   // default on, "0..." switches off
  const char* e = getenv(name);
  return !(e && e[0] == '0');
}
int env_digit(const char* name, int hi, int dflt) {   // one digit 0..hi
  const char* e = getenv(name);
  return (e && e[0] >= '0' && e[0] <= '0' + hi) ? e[0] - '0' : dflt;
}

Knobs read_once() {
  Knobs kn;
  kn.scan_tb = env_on("CRS_SCAN_TB");
  kn.long_chain = env_on("CRS_SCAN_LONG_CHAIN");
  kn.scan_wide = env_on("CRS_SCAN_WIDE");
  kn.scan_w1 = env_on("CRS_SCAN_W1");
  kn.scan_variant = env_digit("CRS_SCAN_VARIANT", 3, 3);
  kn.share_tau = env_digit("CRS_SCAN_SHARE_TAU", 1, 0) == 1;
  kn.scan_boot = env_on("CRS_SCAN_BOOT");
  kn.scan_sched = env_digit("CRS_SCAN_SCHED", 2, 2);
  return kn;
}

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// slots per (query, workgroup) partial list of the Classic kernels: k, or 16 when threshold sharing is on (lists may then be
// dumped unselected)
int partial_width(const Knobs& kn, int k) { return (kn.share_tau && k <= 16) ? 16 : k; }

// the grid of a family's form: all query blocks of a tile stream must be co-resident, so streams = resident slots / query blocks
void lay_out(Plan* p, int64_t n_rows, int cus, int tile_rows, int wg_per_cu, int queries) {
  p->tile_rows = tile_rows;
  p->n_tiles = (int)((n_rows + tile_rows - 1) / tile_rows);
  p->nqb = (p->nq + queries - 1) / queries;
  int streams = cus * wg_per_cu / p->nqb;
  if (streams < 1) streams = 1;
  if (p->nqb > 1 && streams >= 8) streams &= ~7;   // whole rounds over the 8 XCDs (scan_common.h: grid mapping)
  p->nwg = p->n_tiles < streams ? p->n_tiles : streams;
  if (p->nqb > 1 && p->nwg >= 8) p->nwg &= ~7;
}
int tiles_per_stream(const Plan& p) { return (p.n_tiles + p.nwg - 1) / p.nwg; }

// TileBest: short streams send every tile's representative straight to the partial list ("dump", slots 0; merge.hip's
// single-pass path takes <= 8192 candidates per query); longer ones keep the best in a register chain of the returned length.
// -1: no chain holds this k at this row length -- the threshold kernels take the search.
int tile_best_slots(const Plan& p, const Knobs& kn) {
  const int tps = tiles_per_stream(p);
  if ((size_t)tps * p.nwg <= 8192 && tps <= 2 * scan_wide_slots(p.k)) return 0;
  if (p.k <= 16) return scan_wide_slots(p.k);
  const int slots = !kn.long_chain ? 0
                    : p.slab_type == CRS_SLAB_I8 ? scan_i8_long_chain_slots(p.pdim, p.k) : scan_tb_long_chain_slots(p.pdim, p.waves, p.k);
  return slots > 0 ? slots : -1;
}

// What is left once family, form and grid are chosen: the slab stream's cache policy, the dynamic tile schedule, scan.hip's
// bootstrap and schedule, the wide kernel's stagger, MFMA shape and buffer scheme.
int finish_plan(Plan* p, int64_t n_rows, const Knobs& kn) {
  const bool tile_best = p->family == Family::TileBest, wide = p->family == Family::Wide;
  p->part_elems = (size_t)p->nwg * p->nq * p->kp;
  p->share_tau = kn.share_tau;
  // Non-temporal slab stream: a shard's slab far larger than the 256 MB Infinity Cache is read once per launch and replays
  // from nowhere, so its tiles go nt and stop evicting what the encoder lanes beside the sweep re-read; one query block only
  // (several blocks of a launch read every tile several times).  A 77 MB slab (C2) replays from the cache and keeps the default.
  const size_t slab_bytes = (size_t)n_rows * p->pdim * (p->slab_type == CRS_SLAB_I8 ? 1 : 2);
  const bool streamed = tile_best || (wide && scan_wide_streamed(p->k));
  p->nt = !streamed ? 0 : kn.scan_nt >= 0 ? kn.scan_nt : (slab_bytes >= ((size_t)1 << 30) && p->nqb == 1);
  // Dynamic tile schedule of the chain forms (scan_tb.hip, scan_i8.hip, scan_wide.hip's 24- / 32-slot forms): on long streams
  // the last tb_dyn percent of the tiles are drawn from a counter, tb_dyn_g tiles per ticket.  Defaults 85 % in granules of 8
  // (C4 beside the encoder lanes: 44.9 -> 47.2 k q/s on one box; 20 / 50 / 95 / 100 % and granules of 4 / 16 measured within
  // 1 % of that or worse; a ticket per tile is bound by the ~90 M atomics/s one address takes).  One query block only, and the
  // counter lives in the shared-threshold words.  int8 rows of 1024 elements stay static: those instantiations spill, and the
  // ticket's register must not travel through scratch while its value is in flight.
  const bool tb_chain = tile_best && p->slots > 0 && !(p->slab_type == CRS_SLAB_I8 && p->pdim > 768);
  const bool wide_chain = wide && scan_wide_streamed(p->k) && kn.wide_dyn;
  const int rounds = p->n_tiles / p->nwg;
  // (the wide kernel's shape and buffer scheme first: the ring wants one more static round)
  p->mfma = !wide ? 0 : !wide_has_16(p->pdim, p->waves, p->slots) ? 32 : kn.wide_mfma ? kn.wide_mfma : wide_default_mfma(p->pdim, p->slots);
  p->ring = wide && kn.wide_ring && wide_ring_form(p->pdim, p->waves, p->slots, p->mfma);
  p->lds = wide ? scan_wide_lds_bytes(p->pdim, p->waves, p->ring) : 0;
  p->ticket = (tb_chain || wide_chain) && p->nqb == 1 && !kn.share_tau && kn.tb_dyn > 0 &&
              rounds >= (kn.tb_dyn_min < 4 ? 4 : kn.tb_dyn_min);
  p->t_dyn = p->n_tiles;
  p->dyn_mask = 0;
  if (p->ticket) {
    int stat = (int)((int64_t)rounds * (100 - kn.tb_dyn) / 100);   // static rounds ahead of the ticketed ones
    // the kernels know the look-ahead tile of their first iteration without a ticket; the ring kernel looks two tiles ahead
    const int stat_min = p->ring ? 3 : 2;
    if (stat < stat_min) stat = stat_min;
    p->t_dyn = stat * p->nwg;
    p->dyn_mask = kn.tb_dyn_g - 1;
    assert(p->t_dyn >= stat_min * p->nwg && p->t_dyn <= p->n_tiles);
  }
  // short streams only: the bootstrap pays when a workgroup sees few tiles (see scan.hip)
  p->boot = (kn.scan_boot && rounds < 24) ? 1 : 0;
  p->sched = kn.scan_sched;
  p->no_stagger = (wide && !kn.wide_stagger) ? 1 : 0;
  p->no_defer = (wide && !kn.wide_defer) ? 1 : 0;
  return CRS_OK;
}

}  // namespace

Knobs knobs_from_env() {
  static const Knobs once = read_once();
  Knobs kn = once;
  if (const char* e = getenv("CRS_TB_DYN")) { const int v = atoi(e); kn.tb_dyn = v < 0 ? 0 : v > 100 ? 100 : v; }
  if (const char* e = getenv("CRS_TB_DYN_G")) { const int v = atoi(e); kn.tb_dyn_g = v >= 16 ? 16 : v >= 8 ? 8 : v >= 4 ? 4 : v >= 2 ? 2 : 1; }
  if (const char* e = getenv("CRS_TB_DYN_MIN")) kn.tb_dyn_min = atoi(e);
  kn.wide_dyn = env_on("CRS_WIDE_DYN");
  kn.scan_nt = env_digit("CRS_SCAN_NT", 1, -1);
  kn.fused_tail = env_on("CRS_FUSED_TAIL");
  kn.wide_stagger = env_on("CRS_WIDE_STAGGER");
  kn.wide_defer = env_on("CRS_WIDE_DEFER");
  kn.wide_ring = env_on("CRS_WIDE_RING");
  const char* me = getenv("CRS_WIDE_MFMA");
  kn.wide_mfma = !me ? 0 : (me[0] == '1' && me[1] == '6' && !me[2]) ? 16 : (me[0] == '3' && me[1] == '2' && !me[2]) ? 32 : 0;
  return kn;
}

bool Plan::form_exists() const {
  switch (family) {
    case Family::W1: return w1_form_exists(pdim);
    case Family::Wide: return wide_form_exists(pdim, waves, slots, mfma);
    case Family::TileBest: return slab_type == CRS_SLAB_I8 ? i8_form_exists(pdim, slots) : tb_form_exists(pdim, waves, slots);
    default: return slab_type == CRS_SLAB_I8 ? i8_form_exists(pdim, -1) : classic_form_exists(pdim, classic_list_slots(k));
  }
}

// The families in order of preference; the first whose form exists and whose size rules pass takes the search.  The chain forms
// hold k <= 16 (longer chains where scan_forms.h has them); the dump forms (short streams) have no such limit.
int make_plan(int nq, int dim, int k, int64_t n_rows, int slab_type, int cus, const Knobs& kn, Plan* p, const char** why) {
  const auto bad = [&](int code, const char* msg) { *why = msg; return code; };
  if (nq <= 0 || dim <= 0 || dim > 1024) return bad(CRS_EINVAL, "nq must be > 0 and 0 < dim <= 1024");
  if (k <= 0 || k > CRS_MAX_K) return bad(CRS_EINVAL, "k must be in 1..CRS_MAX_K");
  if (n_rows <= 0 || n_rows > 0x7fffffffLL - 64) return bad(CRS_EINVAL, "n_rows must be in 1..2^31-65");
  if (cus <= 0) return bad(CRS_EHIP, "no HIP device available");
  const bool f16 = slab_type == CRS_SLAB_F16;
  const int pdim = row_elems(dim, slab_type);
  *p = Plan{};
  p->slab_type = slab_type;
  p->nq = nq;
  p->k = k;
  p->pdim = pdim;
  p->variant = kn.scan_variant;

  // 1. W1: 65+ queries on 768-element fp16 rows, every tile's representative dumped.  The dump's workspace and merge input grow
  // with the shard (nq * n_rows / 32 entries): past kW1MaxDump entries per (query, stream) -- 1 M rows x 768 at 256 queries is
  // 123 -- the bounded chain kernels below take over (10 M x 768 at 256 queries would otherwise be 640 MB of workspace and 312 k
  // candidates per query)
  if (kn.scan_tb && kn.scan_w1 && f16 && nq > 64 && w1_form_exists(pdim)) {
    p->family = Family::W1;
    p->waves = 8;
    lay_out(p, n_rows, cus, kW1TileRows, kW1WgPerCu, kW1Queries);
    p->kp = tiles_per_stream(*p);
    if (p->kp <= kW1MaxDump) return finish_plan(p, n_rows, kn);
  }
  // 2. Wide: 65+ queries on fp16 rows of <= 512 elements, a register chain of the best tile representatives per lane
  // (16 < k <= 32 on rows of <= 384 elements too: one launch then serves up to 256 queries per sweep at the re-rank's over-fetch)
  if (kn.scan_tb && kn.scan_wide && f16 && nq > 64 && wide_serves(k, pdim)) {
    p->family = Family::Wide;
    p->waves = nq > 128 ? 8 : 4;
    p->slots = scan_wide_slots(k);
    lay_out(p, n_rows, cus, scan_wide_tile_rows(p->waves, pdim), scan_wide_wg_per_cu(p->waves), wide_queries(p->waves));
    p->kp = 2 * p->slots;
    return finish_plan(p, n_rows, kn);
  }
  // 3. TileBest: dump on short streams, chain where one holds k
  if (kn.scan_tb) {
    p->family = Family::TileBest;
    if (f16) {
      p->waves = (nq > 64 && k <= 16 && scan_tb_has_8_waves(pdim)) ? 8 : 4;
      lay_out(p, n_rows, cus, tb_tile_rows(pdim), tb_wg_per_cu(pdim, p->waves), tb_queries(p->waves));
    } else {
      p->waves = 4;
      lay_out(p, n_rows, cus, i8_tile_rows(), classic_wg_per_cu(kn.scan_variant), kI8Queries);
    }
    p->slots = tile_best_slots(*p, kn);
    if (p->slots >= 0) {
      p->kp = p->slots ? p->slots : tiles_per_stream(*p);
      return finish_plan(p, n_rows, kn);
    }
  }
  // 4. Classic: the threshold / compaction kernels, exact lists of rows at any k
  p->family = Family::Classic;
  p->waves = 4;
  p->slots = -1;
  lay_out(p, n_rows, cus, f16 ? classic_tile_rows(pdim) : i8_tile_rows(), classic_wg_per_cu(kn.scan_variant), f16 ? kClassicQueries : kI8Queries);
  p->kp = partial_width(kn, k);
  return finish_plan(p, n_rows, kn);
}

int plan_describe(const Plan& p, char* buf, size_t cap) {
  char name[96];
  if (p.family == Family::W1) snprintf(name, sizeof name, "scan_w2_kernel<%d> (%d queries/workgroup, dump)", p.pdim, kW1Queries);
  else if (p.family == Family::Wide) snprintf(name, sizeof name, "scan_wide_kernel<%d,%d,%d>", p.pdim, p.waves, p.slots);
  else if (p.slab_type == CRS_SLAB_I8)
    snprintf(name, sizeof name, "scan_i8_kernel<%d,%d,%d,%d>", p.pdim, p.tile_rows, p.family == Family::TileBest ? 16 : classic_list_slots(p.k), p.slots);
  else if (p.family == Family::TileBest) snprintf(name, sizeof name, "scan_tb_kernel<%d,%d,%d,%d>", p.pdim, p.tile_rows, p.waves, p.slots);
  else snprintf(name, sizeof name, "scan_f16_kernel<%d,%d,%d>", p.pdim, p.tile_rows, classic_list_slots(p.k));
  return snprintf(buf, cap, "%s streams=%d qblocks=%d kp=%d%s + merge%s", name, p.nwg, p.nqb, p.kp, p.nt ? " nt" : "", p.group_best() ? " + refine" : "");
}

size_t inter_lists(size_t part_elems, int nq) { return part_elems / ((size_t)nq * 4096) + 2; }

WsLayout ws_layout(size_t part_elems, int nq, int k) {
  const size_t inter = (size_t)nq * inter_lists(part_elems, nq) * k;
  size_t off = 0;
  const auto take = [&](size_t bytes) { const size_t at = off; off += align_up(bytes, 256); return at; };
  WsLayout w;
  w.tau = take((size_t)nq * 4);
  w.tau_bytes = off;
  w.part_s = take(part_elems * 4);
  w.part_r = take(part_elems * 4);
  w.win_s = take((size_t)nq * k * 4);
  w.win_i = take((size_t)nq * k * 8);
  w.inter_s = take(inter * 4);
  w.inter_i = take(inter * 8);
  w.bytes = off;
  return w;
}

int plan_workspace_bytes(int nq, int dim, int k, int64_t n_rows, int cus, const Knobs& kn, size_t* bytes, const char** why) {
  Plan p, p8;
  int rc = make_plan(nq, dim, k, n_rows, CRS_SLAB_F16, cus, kn, &p, why);
  if (rc) return rc;
  rc = make_plan(nq, dim, k, n_rows, CRS_SLAB_I8, cus, kn, &p8, why);
  if (rc) return rc;
  // the call does not say which slab type will be searched: cover the plans of both, and the largest grid the
  // threshold kernels can use (resident workgroups), which does not depend on n_rows
  const size_t cap = (size_t)cus * classic_wg_per_cu(kn.scan_variant);
  size_t most = ws_layout(cap * nq * partial_width(kn, k), nq, k).bytes;
  const size_t planned = ws_layout(p.part_elems > p8.part_elems ? p.part_elems : p8.part_elems, nq, k).bytes;
  if (planned > most) most = planned;
  *bytes = most;
  return CRS_OK;
}

}  // namespace crs
