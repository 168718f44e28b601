// scan_stream.h -- the tile stream of the tile-best scans (scan_tb.hip, scan_i8.hip, scan_wide.hip): one definition of the tile
// transfer, the register chain, the ticketed tile schedule's protocol, the partial-list epilogues and the launch.  Each kernel
// keeps its own loop skeleton (where it waits, where its barrier stands) and its own MFMA core.
// Header-only; everything lives in an anonymous namespace of the including translation unit.
#pragma once
#include "scan_common.h"

namespace crs {
namespace {

// ---------------------------------------------------------------- tile transfer
// Global memory -> LDS directly (global_load_lds_dwordx4, 16 bytes per lane; no staging registers, no LDS stores).  The LDS side
// of the transfer is linear -- position P = j * kT + tid of the tile buffer, wave w's 1 KB at +1024 w -- so the XOR swizzle of
// the 16-byte chunks is applied on the SOURCE side: P receives chunk swz(P) (the formula: swizzled_src_offsets, lds_dma.h; every
// fragment read and tail_steps.h's re-score read the tile through the same swizzle).  The transfers are asm (lds_dma.h): the compiler's
// own waitcnt insertion would put a vmcnt(0) in front of every LDS read that may alias an in-flight transfer, i.e. in front of
// every fragment read.
typedef __attribute__((address_space(3))) void* lds_ptr_t;

// this wave's share of tile buffer 0, as the transfers' M0 value (wave-uniform)
__device__ __forceinline__ unsigned tile_lds_wave(char* tile_buf, int wave) {
  return __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_ptr_t)tile_buf + (unsigned)wave * 1024u);
}

// Tile `tile` (wave-uniform) of the slab -> the LDS buffer whose share of this wave starts at dst0.  Full tiles (tile < n_full)
// go from a uniform base, non-temporal where nt (ScanArgs::nt as it comes, an int: a kernel argument, a scalar branch) says so; the ragged last tile clamps every
// lane to the slab's last 16 bytes, last_chunk (rows past the end never rank).  Tile offsets are 64-bit.
template <int kT, int kTileBytes, int kLoads>
__device__ __forceinline__ void stream_tile(const char* slab, int tile, int n_full, size_t last_chunk, unsigned dst0,
                                            const unsigned (&src_off)[kLoads], int nt) {
  if (tile < n_full) {
    const char* base = uniform_ptr(slab + (size_t)tile * kTileBytes);
    if (nt) {
#pragma unroll
      for (int j = 0; j < kLoads; ++j) lds_dma16_nt(dst0 + (unsigned)(j * kT * 16), src_off[j], base);
    } else {
#pragma unroll
      for (int j = 0; j < kLoads; ++j) lds_dma16(dst0 + (unsigned)(j * kT * 16), src_off[j], base);
    }
  } else {
#pragma unroll
    for (int j = 0; j < kLoads; ++j) {
      size_t off = (size_t)tile * kTileBytes + src_off[j];
      off = off > last_chunk ? last_chunk : off;
      const char* p = slab + off;
      const unsigned dst = dst0 + (unsigned)(j * kT * 16);
      lds_dma16(dst, p);
    }
  }
}

// ---------------------------------------------------------------- the chain
// A lane's K best tiles so far as (best score, first row), sorted by score; earlier tile first on ties (strict >).  Empty slots
// are (-inf, -1): the kernels fill ts[] / tr[] with that themselves.
// insert into the sorted list: one branch-free compare-exchange per slot (5 VALU), the loser moves on
template <int K>
__device__ __forceinline__ void chain_insert(float (&ts)[K], int (&tr)[K], float x, int xr) {
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const bool c = x > ts[j];
    const float s_old = ts[j];
    const int r_old = tr[j];
    ts[j] = c ? x : s_old;
    tr[j] = c ? xr : r_old;
    x = c ? s_old : x;
    xr = c ? r_old : xr;
  }
}

// ---------------------------------------------------------------- ticketed tile schedule
// Tile order.  Static part: tiles stream, stream + tstep, ... below t_dyn.  Dynamic part (chain forms, long streams): granules of
// dyn_mask + 1 consecutive tiles from t_dyn + ticket * (dyn_mask + 1), the ticket drawn from a device-wide counter (one address
// takes ~90 M atomics/s on this part: a ticket per tile would be the bottleneck) -- a workgroup that was held up (an encoder
// kernel on its CU, a slower HBM channel) then simply draws fewer tiles instead of making the whole launch wait for its fixed
// share.  The tile AFTER the look-ahead tile tn is requested at the top of an iteration (one lane, one atomic) and handed to the
// workgroup through LDS behind the iteration's barrier: a ticket has a whole tile time (~2 us) to come back.  Any assignment
// gives the same lists after the merge: a workgroup still sees its tiles in increasing order (ties keep the earlier tile).
//
// Is the tile after tn drawn?  It is the static stride, the next tile of tn's granule (in_dyn: tn >= t_dyn), or -- tn is the
// last static tile / the last tile of its granule -- the first tile of the granule the counter hands out (wave-uniform).
__device__ __forceinline__ bool ticket_due(bool in_dyn, int tn, int tstep, int t_dyn, int dyn_mask) {
  return in_dyn ? ((tn - t_dyn) & dyn_mask) == dyn_mask : tn + tstep >= t_dyn;
}
// One lane draws (lane 0 of the wave where `drawer`, wave-uniform, holds; else nobody); tk receives the ticket.  Written as asm
// under a hand-set exec mask: hipcc's atomicAdd waits for the returned value on the spot (its wave-aggregation rewrite reads it
// at once), i.e. for the look-ahead transfer issued just before as well -- transfer and multiplication of the dynamic tiles
// would no longer overlap.  The compiler does not count the asm's memory operation: tk must stay untouched until the caller's
// asm s_waitcnt vmcnt(0) that names it as an operand (tools/check_resources.py audits the assembly for exactly that).
__device__ __forceinline__ void ticket_draw(unsigned& tk, bool drawer, unsigned* ticket) {
  const unsigned mask = __builtin_amdgcn_readfirstlane(drawer ? 1u : 0u);
  unsigned long long keep;
  unsigned zero = 0u, one = 1u;   // (not const: as constants the host pass rejects them as asm operands of a __device__ function)
  asm volatile("s_mov_b64 %1, exec\n\ts_mov_b32 exec_lo, %2\n\ts_mov_b32 exec_hi, 0\n\tglobal_atomic_add %0, %3, %4, %5 sc0\n\ts_mov_b64 exec, %1"
               : "+v"(tk), "=&s"(keep) : "s"(mask), "v"(zero), "v"(one), "s"(ticket) : "memory");
}
// the drawing thread, in front of the iteration's barrier.  Two slots: iteration it + 1 writes the other one
__device__ __forceinline__ void ticket_publish(int* sh_next, int it, unsigned tk, int t_dyn, int dyn_mask) {
  sh_next[it & 1] = t_dyn + (int)tk * (dyn_mask + 1);
}
// every thread, behind the barrier: the granule's first tile, or tend -- a poisoned counter must not become an address
__device__ __forceinline__ int ticket_take(const int* sh_next, int it, int tend) {
  const int tnn = __builtin_amdgcn_readfirstlane(sh_next[it & 1]);
  return (unsigned)tnn < (unsigned)tend ? tnn : tend;
}

// The same pair with the slot named by the caller (scan_wide.hip's ring form keeps a slot per tile buffer: `slot` is its ring index)
__device__ __forceinline__ void ticket_publish_slot(int* sh_next, int slot, unsigned tk, int t_dyn, int dyn_mask) {
  sh_next[slot] = t_dyn + (int)tk * (dyn_mask + 1);
}
__device__ __forceinline__ int ticket_take_slot(const int* sh_next, int slot, int tend) {
  const int tnn = __builtin_amdgcn_readfirstlane(sh_next[slot]);
  return (unsigned)tnn < (unsigned)tend ? tnn : tend;
}

// ---------------------------------------------------------------- partial-list epilogues (scan_tb.hip, scan_i8.hip)
// The query's list starts at slot o of the partial lists [nq, nwg, kp].
// dump form: the slots of tiles this (shorter) stream does not have, shared out over the query's four lanes (first = it + kq)
__device__ __forceinline__ void dump_pad(float* part_s, int* part_r, size_t o, int first, int kp) {
  for (int p = first; p < kp; p += 4) {
    part_s[o + p] = kNegInf;
    part_r[o + p] = -1;
  }
}
// chain form: the list as it stands (kp = K)
template <int K>
__device__ __forceinline__ void chain_store(float* part_s, int* part_r, size_t o, const float (&ts)[K], const int (&tr)[K]) {
#pragma unroll
  for (int j = 0; j < K; ++j) {
    part_s[o + j] = ts[j];
    part_r[o + j] = tr[j];
  }
}

// ---------------------------------------------------------------- launch
// 1-D grid of nqb * nwg workgroups ((query block, tile stream): scan_common.h's grid mapping); the dynamic LDS limit is raised
// once per kernel instantiation.
template <auto kKernel>
int launch_scan(int lds, int threads, const ScanArgs& a, hipStream_t stream) {
  static bool done = false;
  if (!done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kKernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;
    done = true;
  }
  hipLaunchKernelGGL(kKernel, dim3(a.nqb * a.nwg), dim3(threads), lds, stream, a);
  return (int)hipGetLastError();
}

}  // namespace
}  // namespace crs
