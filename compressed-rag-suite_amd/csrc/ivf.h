// ivf.h -- the inverted-file probe: limits, key layout and the plan of one crs_ivf_topk call.  Plain C++ (no HIP), so
// the planner (ivf_plan.cpp) and the kernels (ivf_probe.hip) share one definition.
//
// An IVF index over an fp16 slab is row numbers only: list_offsets int32 [nlist + 1] and list_rows int32 [n] (the slab's rows
// grouped by list, ascending within a list).  A call scores, for each of nq queries, the rows of the nprobe lists named in
// probes int32 [nq, nprobe] (-1 = none) and keeps the kp best of every (query, slot) pair.
//
// Work items.  Pair p = query * nprobe + slot.  The grouping kernel sorts the keys (list << 14 | pair) and cuts the sorted
// sequence where the list changes or a 16th pair of one list is reached: an item is one list and up to 16 pairs that probe it,
// named by the position of its first key.  One workgroup of the probe kernel serves one item, so queries that probe the same
// list share that list's bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace crs {

constexpr int kIvfMaxQ = 256;              // queries of one call
constexpr int kIvfMaxProbe = 64;           // lists per query
constexpr int kIvfPairBits = 14;           // kIvfMaxQ * kIvfMaxProbe = 2^14 pairs
constexpr int64_t kIvfMaxLists = 1 << 18;  // list << 14 | pair fits 32 bits
constexpr int kIvfItemPairs = 16;          // pairs of an item: the 16 columns of the MFMA's B operand
constexpr int kIvfWaves = 4;               // waves of a probe workgroup

// The plan of one call: a pure function of the sizes.
struct IvfPlan {
  int nq, nprobe, kp, k, pdim, ksteps;
  int pairs;            // nq * nprobe: keys, the probe kernel's grid, and the (query, slot) lists of the output
  int sort_n;           // keys the grouping kernel sorts: the power of two >= pairs, at least 64
  int group_threads;    // its one workgroup: min(sort_n, 1024)
  int group_lds;        // sort_n keys + one scan word per thread
  int waves;            // waves of a probe workgroup: they split the list's 16-row tiles
  int ring;             // tiles a wave keeps in flight (registers: ring * ksteps * 4 + ksteps * 4 for the queries)
  int cap;              // keys of a (wave, query) buffer in LDS: 2 kp
  int probe_lds;        // waves * 16 * cap * 8
};
// returns 0, or -1 with *why naming the argument
int ivf_make_plan(int nq, int dim, int nprobe, int k, int kp, int64_t n_rows, int64_t nlist, IvfPlan* p, const char** why);
int ivf_plan_describe(const IvfPlan& p, char* buf, size_t cap);
// workspace: [header: items, valid keys | sorted keys | item starts | pair scores [pairs, kp] | pair rows], 256-byte aligned
struct IvfWs {
  size_t header, keys, items, part_s, part_r, bytes;
};
IvfWs ivf_ws_layout(const IvfPlan& p);

}  // namespace crs
