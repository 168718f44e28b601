// scan_tb.hip -- "tile best" form of the 16x16x32 scan (fp16 slabs; chain form k <= 16, dump form k <= 64): the default for 64-query
// batches, and for larger batches of rows wider than 512 elements (scan_wide.hip takes the others).
//
// scan.hip filters every score against a running per-query threshold, appends survivors to per-lane
// LDS lists and compacts them with in-register sorting networks.  Measured on C2 (100 k rows, 6 tiles
// per workgroup) that machinery -- bootstrap, two in-loop compactions, the final one -- was a third of
// every wave's 57 k cycles and the kernel sat at 0.34 of the HBM roofline; its 80 KB of LDS per workgroup
// also caps residency at two workgroups (two tiles in flight) per CU.
// Here a wave keeps, per query and tile, only the tile's best score (max tree over the lane's
// accumulators + two row swaps across the query's four lanes) filed under the tile's first row; merge.hip
// picks the k best tiles per query and scan_refine.hip re-opens them (exactness argument there):
//   * K = 0, "dump": streams of at most a few tiles write every representative straight to the
//     workgroup's partial list (slot = tile number in the stream);
//   * K > 0, "chain": the representative goes into a register-resident sorted list of the K best so far
//     (branch-free compare-exchange chain, 5 VALU per slot).  All four lanes of a query insert every tile and
//     so hold the same list: letting them take turns (a quarter of the chain work) left a fold of the four
//     lists for the exit -- 200 dependent compare-exchange steps, 37 k cycles during which the workgroup loads
//     nothing, a tenth of the C4 launch -- whereas the chain inside the loop hides behind the memory waits.
// No LDS lists, no data-dependent branch, 2 tiles of LDS per workgroup, two workgroups per CU (TbCfg).  NW = 4 waves serve 64 queries; NW = 8 serve 128 from one
// staged copy of the tile (rows wider than 512 elements, where scan_wide.hip's 32-query fragments no
// longer fit the register file).

#include "scan_stream.h"

namespace crs {
namespace {

template <int D, int TR, int NW>
struct TbCfg {
  static constexpr int kT = NW * 64;
  static constexpr int kCpr = D / 8;
  static constexpr int kTileBytes = TR * D * 2;
  static constexpr int kLoads = kTileBytes / (kT * 16);
  static constexpr int kKsteps = D / 32;
  static constexpr int kRt = TR / 16;
  static constexpr int kLds = 2 * kTileBytes;
  static constexpr int kWgpc = tb_wg_per_cu(D, NW);   // resident workgroups per CU the kernel is built for (scan_forms.h)
  static_assert(D % 128 == 0 && TR % 16 == 0, "row length: multiple of 128 elements; tile rows: multiple of 16");
  static_assert(kTileBytes % (kT * 16) == 0, "tile must split into whole 16-byte loads");
  static_assert(TR == tb_tile_rows(D) && tb_form_exists(D, NW, 0), "scan_forms.h says this geometry does not exist");
};

template <int D, int TR, int NW, int K>
__global__ __launch_bounds__(NW * 64, (TbCfg<D, TR, NW>::kWgpc * NW) / 4) void scan_tb_kernel(const ScanArgs a) {
  using C = TbCfg<D, TR, NW>;
  constexpr int kT = C::kT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* tile_buf = smem;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nwg = CRS_NSTREAMS;
  const int stream = CRS_STREAM;
  WP_DECL;
  const int qbase = CRS_QBLOCK * (NW * 16) + wave * 16;
  const bool wave_active = qbase < a.nq;

  // ---- tile transfer (scan_stream.h).  The offsets are lds_dma.h's swizzled_src_offsets written out: through the helper two
  // kernels of this file lose waits (DESIGN.md section 3.1 has the counts)
  unsigned src_off[C::kLoads];
#pragma unroll
  for (int j = 0; j < C::kLoads; ++j) {
    const int P = j * kT + tid;
    const int r = P / C::kCpr, cp = P % C::kCpr;
    src_off[j] = (unsigned)(r * C::kCpr + ((cp & ~15) | ((cp ^ r) & 15))) * 16u;
  }
  const char* slab = reinterpret_cast<const char*>(a.slab);
  const size_t last_chunk = (size_t)a.n_rows * (D * 2) - 16;
  const int n_full = a.n_rows / TR;
  const unsigned lds_wave = tile_lds_wave(tile_buf, wave);
  auto dma_tile = [&](int tile, int buf) {
    stream_tile<kT, C::kTileBytes>(slab, __builtin_amdgcn_readfirstlane(tile), n_full, last_chunk,
                                   lds_wave + (unsigned)(buf * C::kTileBytes), src_off, a.nt);
  };

#ifdef CRS_TB_CONTIG   /* timing experiment (tools/scan_tb_probe): every stream walks ONE contiguous run of tiles */
  const int tps_ = (a.n_tiles + nwg - 1) / nwg;
  const int tstep = 1, tend = min(a.n_tiles, (stream + 1) * tps_);
  int t = stream * tps_;
#else
  const int tstep = nwg, tend = a.n_tiles;
  int t = stream;
#endif
  // Tile order: static stride below t_dyn, then (chain mode, long streams) ticketed granules -- scan_stream.h, "Tile order"
  __shared__ int sh_next[2];
  const int t_dyn = K > 0 ? a.t_dyn : a.n_tiles;
  int tn = t + tstep;     // the look-ahead tile (t_dyn >= 2 nwg: static for the first iteration)
  dma_tile(t, 0);   // before the query fragments are fetched: the two latencies overlap
  const int lr = lane & 15, kq = lane >> 4;
  const int qi = qbase + lr;
  const bool q_valid = qi < a.nq;
  f16x8 qf[C::kKsteps];
  {
    const _Float16* qrow = a.q + (size_t)(q_valid ? qi : 0) * D + kq * 8;
#pragma unroll
    for (int ks = 0; ks < C::kKsteps; ++ks) {
      const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      qf[ks] = q_valid ? *reinterpret_cast<const f16x8*>(qrow + ks * 32) : z;
    }
#pragma unroll
    for (int ks = 0; ks < C::kKsteps; ++ks) {
      f16x8 x = qf[ks];
      asm volatile("" : "+v"(x));
      qf[ks] = x;
    }
  }
  int a_off[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) a_off[m] = lr * (C::kCpr * 16) + (((m * 4 + kq) ^ lr) & 15) * 16;
  // the query's slots in the partial list [nq, nwg, kp]
  const size_t o = ((size_t)(q_valid ? qi : 0) * nwg + stream) * a.kp;
  float* out_s = a.part_scores + o;
  int* out_i = a.part_rows + o;

  // chain mode: this lane's K best tiles so far as (best score, first row), sorted; earlier tile first on ties
  constexpr int KK = K > 0 ? K : 1;
  float ts[KK];
  int tr[KK];
#pragma unroll
  for (int j = 0; j < KK; ++j) { ts[j] = kNegInf; tr[j] = -1; }
  // (through a lambda, as the local chain was: called from the loop directly, the chain forms grow by up to 24 scalar instructions)
  auto insert = [&](float x, int xr) { chain_insert(ts, tr, x, xr); };

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  WP_LAP(0);   // prologue

  int cur = 0, it = 0;
  // one iteration: tile t sits in LDS buffer `cur`; tile t + nwg streams into the other buffer while t is multiplied
  while (t < tend) {
    const bool has_next = tn < tend;
    if (has_next) dma_tile(tn, cur ^ 1);
    const bool in_dyn = K > 0 && tn >= t_dyn;
    const bool draw = K > 0 && a.ticket != nullptr && ticket_due(in_dyn, tn, tstep, t_dyn, a.dyn_mask);
    unsigned tk = 0;   // the ticket in flight: first read behind the vmcnt(0) below
    if constexpr (K > 0) ticket_draw(tk, draw && has_next && wave == 0, a.ticket);
    WP_LAP(1);   // look-ahead issue
#if defined(CRS_TB_EXPERIMENT) && CRS_TB_EXPERIMENT <= 2   /* tools/scan_tb_probe.hip: timing-only builds (1: no MFMA / selection, 3: fragment reads without MFMA, 4: MFMA without fragment reads) */
    if (false) {
#else
    if (wave_active) {
#endif
      const char* buf = tile_buf + cur * C::kTileBytes;
      float best = kNegInf;
#pragma unroll
      for (int rt = 0; rt < C::kRt; ++rt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < C::kKsteps; ++ks) {
#if defined(CRS_TB_EXPERIMENT) && CRS_TB_EXPERIMENT == 3
          const f32x4 af = *reinterpret_cast<const f32x4*>(buf + a_off[ks & 3] + rt * 16 * (C::kCpr * 16) + (ks >> 2) * 256);
          acc[ks & 3] += af[ks & 3];
#elif defined(CRS_TB_EXPERIMENT) && CRS_TB_EXPERIMENT == 4
          acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(qf[(ks + rt) % C::kKsteps], qf[ks], acc, 0, 0, 0);
#else
          const f16x8 af = *reinterpret_cast<const f16x8*>(buf + a_off[ks & 3] + rt * 16 * (C::kCpr * 16) + (ks >> 2) * 256);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, qf[ks], acc, 0, 0, 0);
#endif
        }
        if (t < n_full) {
          best = fmaxf(best, fmaxf(fmaxf(acc[0], acc[1]), fmaxf(acc[2], acc[3])));
        } else {   // ragged last tile: rows past the end must not win
          const int row0 = t * TR + rt * 16 + kq * 4;
#pragma unroll
          for (int i = 0; i < 4; ++i) best = (row0 + i < a.n_rows) ? fmaxf(best, acc[i]) : best;
        }
      }
      WP_LAP(3);   // fragment reads + MFMA
      best = quad_max(best);   // the query's four lanes: all rows of the tile
      if constexpr (K == 0) {
        if (q_valid && kq == 0) {
          out_s[it] = best;
          out_i[it] = t * TR;
        }
      } else {
        insert(best, t * TR);   // all four lanes of the query: they hold the same list, so nothing is left to fold at the exit
      }
    }
    WP_LAP(4);   // selection
    int tnn = in_dyn ? tn + 1 : tn + tstep;
    if (has_next) {
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(tk) : : "memory");
      WP_LAP(5);   // wait for the look-ahead tile (and for the ticket)
      if (K > 0 && draw && tid == 0) ticket_publish(sh_next, it, tk, t_dyn, a.dyn_mask);
      __syncthreads();
      WP_LAP(7);   // barrier
      if (K > 0 && draw) tnn = ticket_take(sh_next, it, tend);
    }
    cur ^= 1;
    ++it;
    t = tn;
    tn = tnn;
  }
  if (wave_active) {
    if constexpr (K == 0) {
      if (q_valid) dump_pad(out_s, out_i, 0, it + kq, a.kp);
    } else {
      if (q_valid && kq == 0) chain_store(out_s, out_i, 0, ts, tr);
    }
  }
  WP_LAP(10);   // final fold + write
  WP_STORE(NW);
}

__global__ void tb_zero_ticket_kernel(unsigned* ticket) {
  if (threadIdx.x < 4) ticket[threadIdx.x] = 0u;
}

template <int D, int TR, int NW, int K>
int launch_tb(const ScanArgs& a, hipStream_t stream) {
  return launch_scan<&scan_tb_kernel<D, TR, NW, K>>(TbCfg<D, TR, NW>::kLds, NW * 64, a, stream);
}

// the form if scan_forms.h has it
template <int D, int TR, int NW, int K>
int launch_tb_if(const ScanArgs& a, hipStream_t stream) {
  if constexpr (tb_form_exists(D, NW, K)) return launch_tb<D, TR, NW, K>(a, stream);
  else return -1;
}

template <int D, int TR, int NW>
int launch_tb_k(const ScanArgs& a, int slots, hipStream_t stream) {
  switch (slots) {
    case 0: return launch_tb_if<D, TR, NW, 0>(a, stream);
    case 4: return launch_tb_if<D, TR, NW, 4>(a, stream);
    case 10: return launch_tb_if<D, TR, NW, 10>(a, stream);
    case 16: return launch_tb_if<D, TR, NW, 16>(a, stream);
    // 16 < k <= 64 on long streams: a longer chain (5 VALU per slot and tile, still under the tile's memory time) instead of the
    // threshold kernels.  10 M x 384, 64 queries, k = 17 / 32: scan 2.36 / 2.13 ms on the threshold kernels -> 1.23 ms, whole
    // search 2.09 / 2.16 -> 1.31 / 1.32.  24: the store's over-fetch on large shards.
    case 24: return launch_tb_if<D, TR, NW, 24>(a, stream);
    case 32: return launch_tb_if<D, TR, NW, 32>(a, stream);
    case 64: return launch_tb_if<D, TR, NW, 64>(a, stream);
    case 56: return launch_tb_if<D, TR, NW, 56>(a, stream);
    case 48: return launch_tb_if<D, TR, NW, 48>(a, stream);
    case 40: return launch_tb_if<D, TR, NW, 40>(a, stream);
    default: return -1;
  }
}

template <int D, int TR>
int launch_tb_d(const ScanArgs& a, int nw, int slots, hipStream_t stream) {
  if constexpr (scan_tb_has_8_waves(D)) {
    if (nw == 8) return launch_tb_k<D, TR, 8>(a, slots, stream);
  }
  return nw == 4 ? launch_tb_k<D, TR, 4>(a, slots, stream) : -1;
}

}  // namespace

// slots = 0: dump mode (kp = tiles per stream); else chain mode with that many slots (kp = slots)
// the ticket counter is zeroed by a kernel of our own, in stream order: a kernel node in a captured graph like the scan itself
// (a hipMemsetAsync node gave correct lists too, but split the graph's event timing)
int scan_ticket_zero(unsigned* ticket, hipStream_t stream) {
  hipLaunchKernelGGL(tb_zero_ticket_kernel, dim3(1), dim3(64), 0, stream, ticket);
  return (int)hipGetLastError();
}

int scan_launch_tb(const ScanArgs& a, int pdim, int nw, int slots, hipStream_t stream) {
  switch (pdim) {
    case 128: return launch_tb_d<128, 32>(a, nw, slots, stream);
    case 256: return launch_tb_d<256, 32>(a, nw, slots, stream);
    case 384: return launch_tb_d<384, 32>(a, nw, slots, stream);
    case 512: return launch_tb_d<512, 32>(a, nw, slots, stream);
    case 640: return launch_tb_d<640, 16>(a, nw, slots, stream);
    case 768: return launch_tb_d<768, 16>(a, nw, slots, stream);
    case 896: return launch_tb_d<896, 16>(a, nw, slots, stream);
    case 1024: return launch_tb_d<1024, 16>(a, nw, slots, stream);
    default: return -1;
  }
}

}  // namespace crs
