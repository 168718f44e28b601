// merge_sorted.hip -- merge of SORTED top-k lists by co-ranking (gfx950): crs_merge_sorted / crs_merge_sorted_wire.
//
// The cross-shard merge above merge.hip's 64: every shard hands in its exact top-k, k up to CRS_MAX_K_CERT, ALREADY in the
// order of the tail (before(): score desc, id asc; empty slots (-inf, -1) at the end), and ids >= 0 are distinct across lists
// (global sidecar rows).  merge_kernel also serves unsorted dump lists, selects by a threshold and ranks in LDS, which is why
// it stops at k = 64; sorted input needs none of that:
//
//     slot(entry at position p of list r) = p + sum over r' != r of c(r'),
//     c(r') = entries of list r' that are not after it (r' < r)  /  that are strictly before it (r' > r)
//
// is a bijection from the nlists * k_in entries onto [0, nlists * k_in) even among equal keys, and each c(r') is one binary
// search in a sorted list.  No sort, no atomics, no workgroup waits for another: every output slot below nlists * k_in is
// written by exactly one entry, the slots past it (fewer inputs than outputs) by the workgroups of list 0.
// Empty slots take part like entries: they order after every valid entry whatever their score bits and among themselves by
// (list, position), and they write (-inf, -1).
//
// Only the first kk = min(k_in, k_out) entries of a list can land below k_out or be counted below it (a count that reaches kk
// already puts the slot at or past k_out), so lists are read and searched to kk only.
//
// One 256-thread workgroup per (query, list): nq x nlists workgroups keep the CUs busy at nq = 1 .. 64.  A thread owns up to
// four entries of its list in registers; the other lists pass through LDS in groups of <= kCap entries (one cooperative load
// with everything in flight, then searches at LDS latency, a thread's four searches interleaved step by step).

#include "scan.h"
#include "tail_steps.h"

namespace crs {
namespace {

constexpr int kThreads = 256;
constexpr int kOwn = 4;       // entries per thread: kThreads * kOwn >= CRS_MAX_K_CERT
constexpr int kCap = 4096;    // LDS entries per group of lists (48 KB): >= 4 lists at kk = 1024
static_assert(kThreads * kOwn >= 1024 && kCap >= 1024, "a list of CRS_MAX_K_CERT entries must fit");

// Does entry (s2, id2) of list r2 come ahead of (s, id) of list r in the merged order?  earlier = (r2 < r).
__device__ __forceinline__ bool sorted_ahead(float s2, int64_t id2, float s, int64_t id, bool earlier) {
  if (id2 < 0) return id < 0 && earlier;     // empty slots: after every valid entry, among themselves by list
  if (id < 0) return true;
  return earlier ? !before<int64_t>(s, id, s2, id2) : before<int64_t>(s2, id2, s, id);
}

__global__ __launch_bounds__(kThreads) void merge_sorted_kernel(const float* __restrict__ scores, const int64_t* __restrict__ ids, int nlists,
                                                                int k_in, int k_out, size_t list_stride, size_t id_list_stride,
                                                                float* __restrict__ out_s, int64_t* __restrict__ out_i) {
  __shared__ float sh_s[kCap];
  __shared__ int64_t sh_i[kCap];

  const int q = blockIdx.x / nlists, r = blockIdx.x - q * nlists;
  const int tid = threadIdx.x;
  const int kk = k_in < k_out ? k_in : k_out;
  const int n_own = (kk + kThreads - 1) / kThreads;          // <= kOwn (uniform)
  const float* qs = scores + (size_t)q * k_in;               // list l of the query: qs + l * list_stride
  const int64_t* qi = ids + (size_t)q * k_in;
  float* os = out_s + (size_t)q * k_out;
  int64_t* oi = out_i + (size_t)q * k_out;

  // this thread's entries of list r (position tid + kThreads u), and their counts so far
  float s[kOwn];
  int64_t id[kOwn];
  int cnt[kOwn];
#pragma unroll
  for (int u = 0; u < kOwn; ++u) {
    const int p = tid + kThreads * u;
    const bool in = p < kk;
    s[u] = in ? qs[(size_t)r * list_stride + p] : kNegInf;
    id[u] = in ? qi[(size_t)r * id_list_stride + p] : (int64_t)-1;
    cnt[u] = 0;
  }
  int top = 1;                                               // largest power of two <= kk
  while (top * 2 <= kk) top *= 2;

  const int per = kCap / kk;                                 // lists per LDS group (>= 4)
  for (int l0 = 0; l0 < nlists; l0 += per) {
    const int nl = (nlists - l0 < per) ? nlists - l0 : per;
    if (l0 > 0) __syncthreads();                             // the previous group's searches are done
    for (int e = tid; e < nl * kk; e += kThreads) {
      const int l = e / kk, slot = e - l * kk;
      sh_s[e] = qs[(size_t)(l0 + l) * list_stride + slot];
      sh_i[e] = qi[(size_t)(l0 + l) * id_list_stride + slot];
    }
    __syncthreads();
    for (int l = 0; l < nl; ++l) {
      if (l0 + l == r) continue;                             // (uniform)
      const bool earlier = l0 + l < r;
      const float* ls = sh_s + l * kk;
      const int64_t* li = sh_i + l * kk;
      // c = the largest j in [0, kk] with entry j - 1 ahead of ours (the list is sorted: "ahead" is true, then false)
      int c[kOwn] = {0, 0, 0, 0};
      for (int step = top; step > 0; step >>= 1) {
#pragma unroll
        for (int u = 0; u < kOwn; ++u) {
          if (u < n_own) {                                   // (uniform)
            const int j = c[u] + step;
            const int at = (j <= kk ? j : kk) - 1;
            if (j <= kk && sorted_ahead(ls[at], li[at], s[u], id[u], earlier)) c[u] = j;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kOwn; ++u) cnt[u] += c[u];
    }
  }

#pragma unroll
  for (int u = 0; u < kOwn; ++u) {
    const int p = tid + kThreads * u;
    const int slot = p + cnt[u];
    if (p < kk && slot < k_out) {
      os[slot] = id[u] >= 0 ? s[u] : kNegInf;
      oi[slot] = id[u] >= 0 ? id[u] : (int64_t)-1;
    }
  }
  // fewer inputs than outputs (then kk == k_in): the slots no entry maps to
  if (r == 0)
    for (int slot = nlists * kk + tid; slot < k_out; slot += kThreads) { os[slot] = kNegInf; oi[slot] = -1; }
}

int launch(const float* scores, const int64_t* ids, int nlists, int nq, int k_in, int k_out, size_t list_stride, size_t id_list_stride,
           float* out_scores, int64_t* out_ids, hipStream_t stream) {
  hipLaunchKernelGGL(merge_sorted_kernel, dim3((unsigned)nq * (unsigned)nlists), dim3(kThreads), 0, stream, scores, ids, nlists, k_in,
                     k_out, list_stride, id_list_stride, out_scores, out_ids);
  return (int)hipGetLastError();
}

}  // namespace

// all-gather layout: [nlists, nq, k_in]
int merge_sorted_launch_i64(const float* scores, const int64_t* ids, int nlists, int nq, int k_in, int k_out, float* out_scores,
                            int64_t* out_ids, hipStream_t stream) {
  return launch(scores, ids, nlists, nq, k_in, k_out, (size_t)nq * k_in, (size_t)nq * k_in, out_scores, out_ids, stream);
}

// wire layout (crs_hip.h): nlists blocks of `block_bytes`, each [ids int64 [nq, k_in] | scores fp32 [nq, k_in] | pad]
int merge_sorted_launch_wire(const void* wire, size_t block_bytes, size_t scores_off, int nlists, int nq, int k_in, int k_out,
                             float* out_scores, int64_t* out_ids, hipStream_t stream) {
  const int64_t* ids = reinterpret_cast<const int64_t*>(wire);
  const float* scores = reinterpret_cast<const float*>(reinterpret_cast<const char*>(wire) + scores_off);
  return launch(scores, ids, nlists, nq, k_in, k_out, block_bytes / 4, block_bytes / 8, out_scores, out_ids, stream);
}

}  // namespace crs
