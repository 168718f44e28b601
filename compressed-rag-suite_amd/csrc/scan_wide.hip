// scan_wide.hip -- the exact cosine scan for LARGE query batches (65 .. 256 queries per workgroup).
//
// scan.hip serves 64 queries per workgroup: 4 waves x 16 queries, one ds_read_b128 of the slab tile
// per v_mfma_f32_16x16x32_f16.  A batch of 256 queries (BASELINE config #3, and every N-GPU step,
// where each rank scans its shard for the queries of ALL ranks) then needs four workgroups per tile
// stream, i.e. four stagings of every tile (L2 -> VGPR -> LDS) and four times the LDS reads: measured
// on C3 (1 M x 768, 256 queries) that path ran at 23 % MFMA / 36 % LDS / 48 % HBM utilisation with the
// waves parked 47 % of the time -- latency-bound on the re-staging, not on any pipe.
//
// Here ONE workgroup of NW = 4 or 8 waves serves 32 * NW queries from ONE staged copy of the tile:
//   * v_mfma_f32_32x32x16_f16, A = 32 slab rows of the tile (LDS), B = the wave's 32 queries, whose
//     fragments for the full depth D stay in VGPRs for the whole kernel (D/4 registers);
//     one ds_read_b128 now feeds 32 MFMA cycles instead of 16, and a tile is staged once per 256 queries;
//   * result layout: lane l holds query (l & 31), rows (reg & 3) + 8 (reg >> 2) + 4 (l >> 5) of the tile:
//     16 rows of the tile per lane, a query's scores live in a lane PAIR (l, l ^ 32);
//   * selection is "tile best" (scan_refine.hip): per tile the lane pair reduces its 2 x 16 scores to the
//     tile's best row (one xor-shuffle), and that single candidate is inserted into a register-resident
//     sorted list of the K best so far (a branch-free compare-exchange chain, 5 VALU per slot).  Nothing is
//     filtered against a threshold, no LDS lists, no compaction.  Chains of up to 16 slots: the two lanes of
//     a pair take turns -- lane half h inserts the tiles of parity h into its own K-slot list -- so the
//     chain runs once per TWO tiles.  Chains of 24 / 32 slots: ONE K-slot list per lane pair, split across
//     it ("Split list" below) -- K / 2 slots per lane, the chain runs every tile on both halves at once;
//     The first version of this kernel used scan.hip's per-lane LDS candidate lists + wave compaction:
//     measured on C4 with 256 queries (tools/scan_wide_probe), of 1.13 M cycles per wave 0.38 M went to
//     compactions (15 k cycles each, and with 8 waves behind one barrier every one of them stalls the
//     workgroup), 0.26 M to the 16 data-dependent appends per tile and 0.24 M to the MFMAs.
//     At the end every lane writes its K (score, row) pairs; merge.hip picks the k best representatives
//     over all workgroups and scan_refine.hip re-opens their row groups;
//   * tile staging, XOR swizzle (conflict-free for the 32-row fragment reads too: every 16-lane group of
//     a ds_read_b128 covers 16 distinct rows mod 16), early asm loads and the one-barrier double buffer
//     are those of scan.hip.
// Chains of 4 / 10 / 16 slots per lane, and 24 / 32 for rows of <= 384 elements (the over-fetch of the fp32 re-rank on large
// shards is 24: one launch then serves the four 64-query batches of a fused search chunk from ONE sweep of the shard).  The 24- /
// 32-slot forms run one query block per launch in practice, so they also take scan_tb.hip's non-temporal slab stream and its
// ticketed dynamic tile schedule behind the same plan fields (ScanArgs::nt, ticket / t_dyn / dyn_mask); the shorter chains are
// compiled without either, exactly as they were measured.
//
// Split list (K = 24, 32).  The lower half of a lane pair (h = 0) holds ranks 0 .. K/2 - 1 of the pair's list, the upper half
// ranks K/2 .. K - 1.  Per tile the upper half fetches the lower half's LAST slot as it is before the insertion (one
// v_permlane32_swap each for score and row), the lower half inserts the tile's (x, row), and the upper half inserts what the lower
// half pushes out: its old last slot where x > that slot, else x itself.  Both halves insert by SHIFTING (insert_shift below): every
// slot that x beats (strict >: a later tile goes behind an equal earlier one) moves down one place, whatever it holds -- the compare-
// exchange chain of the shorter forms lets a displaced entry step over an equal one, and then what falls off a half's end is no longer
// its last slot.  The shift keeps the pair's list in the order (score desc, earlier tile first) exactly: a pushed-out slot is >= every
// entry of the upper half and earlier than the equal ones, x beats all of those, so it lands in front of them; until the lower half
// is full the upper half is handed (-inf, -1), a no-op.  The K best tiles of the shard that a workgroup saw are among that one
// list as they were among its two parity lists.  VALU per tile is what it was (K/2 x 5 every tile against K x 5 every second tile,
// + 6 for the exchange); the list's registers halve, which is what lets <384, 8, 24> keep the deferred accumulators of the stagger
// (wide_stagger<>).
//
// Deferred insertion (the split forms of wide_defer<>).  The chain above runs for every lane on every tile, yet tile i of a stream
// enters a K-slot list with probability about K / i.  So each lane keeps ONE pending tile (pend_s, pend_r) and a bound thr: the
// upper half's last slot -- the pair's K-th score -- as it stood after the last chain run, in both lanes of the pair (-inf until the
// list is full, so the first K tiles of a stream run the chain every tile as before).  Per tile: x is a candidate where x > thr
// (strict).  If any lane of the WAVE has a candidate and a taken slot (one ballot, a scalar branch), the whole wave first runs the
// chain on its pending entries ("flush"; an empty slot inserts (-inf, -1), which beats nothing), refreshes thr by one more swap and
// re-tests; the candidates are then stashed.  One flush after the last tile (for waves 4 .. 7: after the deferred last tile).
// The lists stay bit for bit what the chain on every tile leaves.  (1) A tile that is not stashed has x <= thr, and thr <= every
// slot of the pair's list now and later, because the K-th score only rises: insert_shift moves nothing for such an x (its compares
// are the same strict >), nor for a NaN, which is never a candidate either.  (2) A lane's stashed tiles reach the chain in the order
// of their tiles, each before any later tile of that lane is stashed, and insert_shift's result for an entry depends only on the
// list it meets -- which by (1) is the list the undeferred code would hold at that tile, skipped tiles being no-ops there.  So the
// sequence of insertions that change the list, and with it the order of equal scores, is the undeferred one.  A wave-wide skip
// alone does not pay (32 lists per wave: on 610-tile streams 9 tiles in 10 have a candidate somewhere); with the slot the chain runs
// on about half the tiles.  CRS_WIDE_DEFER=0 (ScanArgs::no_defer) runs the chain on every tile: A/B runs, and the tests' reference.

//
// 16x16x32 form (scan_wide16_kernel; the split-list forms of the 8-wave kernel on 256- / 384-element rows).  The same launch on
// v_mfma_f32_16x16x32_f16: staging, tile schedule, tickets, nt stream, stagger and the partial-list layout are those above (one
// body, scan_wide_body<.., S16>); what differs is the arithmetic's shape and, with it, which lanes hold what.
//   * a wave's 32 queries are two column groups g of 16; lane (n = l & 15, kq = l >> 4) holds Q[16 g + n][32 ks + 8 kq .. + 8]
//     for both groups and every k-step ks < D / 32 -- the same D / 4 registers;
//   * the A fragment is scan_tb.hip's: row 16 rt + (l & 15) of the tile's four 16-row blocks, chunk 4 ks + kq through the same
//     swizzle; every fragment read feeds two MFMAs, one per group.  The k-step is the OUTER loop, so eight accumulators
//     (4 row blocks x 2 groups) are in flight and no MFMA waits for its neighbour, and the fragments of k-step ks + 1 are read
//     while those of ks are multiplied (pinned with sched_group_barrier: one ds_read_b128 per pair of MFMAs);
//   * each accumulator sums its k-steps in ascending order from zero: tile_rescore_f16's arithmetic (tail_steps.h), so a
//     representative is bit for bit the score the tail's re-score gives its row;
//   * result layout: lane (n, kq) holds rows 16 rt + 4 kq + i of the tile for queries n and 16 + n.  The lane quad of column n
//     serves both: lanes kq = 0, 1 keep the split list of group 0's query, lanes 2, 3 of group 1's -- the pair is (l, l ^ 16),
//     kq & 1 the half, and the lower half's last slot crosses by v_permlane16_swap instead of v_permlane32_swap.  The list
//     algorithm (insert_shift) and its proof are unchanged: they only speak of "the two lanes of the pair".
// Which shape a form runs is wide_default_mfma() (scan_forms.h), set from A/B runs by wall time; CRS_WIDE_MFMA=16 | 32 overrides it.
//
// Ring form (wide_ring<>; the kernels are compiled in scan_wide_ring.hip, which includes this file).  The loop above keeps two tile
// buffers and ends every iteration in s_waitcnt vmcnt(0) + __syncthreads(): all eight waves issue their six transfers of the
// look-ahead tile together at the top of an iteration, straight behind the barrier.  Both waves of every SIMD then sit in transfer
// issue at once (no MFMA runs on the CU meanwhile), and waves 4 .. 7 queue behind waves 0 .. 3 in the CU's one texture addresser --
// time that waves 0 .. 3 then spend at the barrier (profiles/r14_wide_probe.txt: issue 794 / 1470 cycles, barrier 920 / 337 of a
// 4.88 k-cycle tile).  The ring form changes where the transfers are issued and how the buffers rotate, nothing else:
//   * three tile buffers; iteration i multiplies tile T[i] out of buffer i mod 3, and the transfer of T[i + 2] is issued DURING
//     iteration i into buffer (i + 2) mod 3, whose last reads (of T[i - 1]) lie behind barrier i - 1, which every wave has passed;
//   * each wave keeps "s_waitcnt vmcnt(0), then issue my six transfers of T[i + 2]": at most one tile in flight per wave, but it
//     stays in flight across the barrier.  Waves 0 .. 3 do it behind their selection (in what was barrier wait), waves 4 .. 7
//     between their deferred selection and their MFMA sweep: on every SIMD one wave multiplies while its partner is held in issue,
//     and the halves no longer meet in the texture addresser.  A wave's vmcnt(0) in iteration i retires its share of T[i + 1],
//     issued a whole iteration earlier; it precedes barrier i and T[i + 1] is first read behind that barrier;
//   * the iteration ends in s_waitcnt lgkmcnt(0) + a raw s_barrier: __syncthreads()'s fence waits vmcnt(0), which would drain the
//     transfer just issued.  Every wave reaches the barrier on every iteration (idle waves issue their share of each tile too);
//   * tickets: (t, tn, tnn) are known at the top of an iteration and wave 0 draws the tile after tnn there, ahead of its
//     transfers in program order; its vmcnt(0) in front of its issue is the one that names the ticket's register, the drawing
//     thread publishes behind it and ahead of the barrier (one slot per tile buffer), every thread takes behind the barrier.  The
//     first three tiles of a stream are static (plan.cpp: t_dyn >= 3 nwg for these plans);
//   * streams of one or two tiles issue nothing past their end; nothing is in flight when the loop is left.
// The lists are those of the two-buffer kernel bit for bit: tiles reach select() in the same order with the same accumulators.
// CRS_WIDE_RING=0 (Plan::ring) launches the form's two-buffer kernel: A/B runs, and the tests' reference.

#include "scan_stream.h"

namespace crs {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// rows per tile: 32 * RB (RB 32x32 MFMA row blocks).  The 8-wave kernel takes 64-row tiles where the registers
// allow: the per-tile costs that are not MFMAs (barrier, selection chain, load issue, LDS store: ~1.9 k cycles
// per wave and 32-row tile against 1.5 k of matrix work) are then paid once per 64 rows.
template <int D, int NW>
constexpr int wide_rb() { return scan_wide_tile_rows(NW, D) / 32; }

// the forms with chains longer than 16 slots: nt stream + dynamic tile schedule compiled in (header)
template <int K>
constexpr bool wide_streamed() { return K > 16; }
// the same forms keep one K-slot list per lane pair, K / 2 slots in each half (header: "Split list")
template <int K>
constexpr bool wide_split() { return K > 16; }
template <int K>
constexpr int wide_lane_slots() { return wide_split<K>() ? K / 2 : K; }
// Waves 4..7 defer a tile's selection by one iteration (the stagger below) where the deferred accumulators fit: two waves per
// SIMD leave 256 registers per lane, VGPRs and AGPRs together.  384-element rows: 96 of query fragments, 32 + 32 of current and
// deferred accumulators and 2 x (slots per lane) of chain -- 16 slots per lane and more would spill
// (profiles/r07_wide_resources.txt).  The split list leaves <384, 8, 24> 12 slots per lane: 256 registers, no scratch
// (profiles/r12_wide_resources.txt).  The other forms keep the value they were measured with.
template <int D, int NW, int K>
constexpr bool wide_stagger() {
  if (D == 384 && NW == 8 && K == 24) return true;
  return NW == 8 && D <= 384 && !(D == 384 && K >= 16) && !(D == 256 && K >= 32);
}
// The split forms whose chain is deferred behind a pending slot per lane (header: "Deferred insertion"): the ones measured faster
// with it by the rule of DESIGN.md section 7 item 6; every other form is compiled with the chain on every tile, as it was measured.
// -DCRS_WIDE_DEFER_ALL=1 compiles the deferral into every split form (A/B builds of tools/scan_wide_probe and tools/wide_defer_ab).
#ifndef CRS_WIDE_DEFER_ALL
#define CRS_WIDE_DEFER_ALL 0
#endif
// The 32x32x16 form of <384, 8, 24> sits at 256 registers: the three of the pending slot spill (8 bytes per lane), so it never defers.
template <int D, int NW, int K, bool S16>
constexpr bool wide_defer() {
  if (!wide_split<K>() || (!S16 && D == 384 && NW == 8 && K == 24)) return false;
  if (CRS_WIDE_DEFER_ALL) return true;
  return S16 && D == 384 && NW == 8 && K == 24;
}

// The forms that have a ring kernel (header: "Ring form"; scan_forms.h decides, so that the planner knows them too)
template <int D, int NW, int K, bool S16>
constexpr bool wide_ring() { return wide_ring_form(D, NW, K, S16 ? 16 : 32); }

template <int D, int NW>
struct WCfg {
  static constexpr int kThreadsW = NW * 64;
  static constexpr int kCpr = D / 8;
  static constexpr int RB = wide_rb<D, NW>();
  static constexpr int TR = 32 * RB;
  static constexpr int kTileBytes = TR * D * 2;
  static constexpr int kLoads = kTileBytes / (kThreadsW * 16);
  static constexpr int kKsteps = D / 16;
  static constexpr int kQStage = NW * 4096;   // prologue: 4 KB per wave for the query transpose, in the last tile buffer
  static constexpr int kLds = 2 * kTileBytes > kTileBytes + kQStage ? 2 * kTileBytes : kTileBytes + kQStage;
  static constexpr int kLdsRing = scan_wide_lds_bytes(D, NW, true);   // three buffers
  static_assert(kLds == scan_wide_lds_bytes(D, NW, false), "the planner's LDS bytes are the launch's");
  static_assert(D % 128 == 0, "row length must be a multiple of 128 elements");
  static_assert(kTileBytes % (kThreadsW * 16) == 0, "tile must split into whole 16-byte loads");
};

// a tile's scores in one wave: 32x32x16 -- RB blocks of 32 rows x 32 queries; 16x16x32 -- 2 RB blocks of 16 rows x 2 groups of 16 queries
template <int RB, bool S16>
struct WAcc { f32x16 a[RB]; };
template <int RB>
struct WAcc<RB, true> { f32x4 a[2 * RB][2]; };

// The body of both kernels; S16 picks the compute form (MFMA shape, fragment layout, which lanes hold a query's list).
// The arguments come by value as they come to a kernel: taken by reference, scan_wide_kernel<384, 8, 24> spilled 20 bytes per lane.
// RING: the three-buffer loop (header: "Ring form").  (A second look-ahead tile behind the two-buffer loop's vmcnt(0) +
// __syncthreads() measured no faster, but that barrier drains every transfer in flight, so it never tested a transfer that spans it.)
template <int D, int NW, int K, bool S16, bool RING = false>
__device__ __forceinline__ void scan_wide_body(const ScanArgs a) {
  using C = WCfg<D, NW>;
  static_assert(!RING || (wide_ring<D, NW, K, S16>() && wide_streamed<K>()), "no ring kernel for this form");
  static_assert(!S16 || wide_has_16(D, NW, K), "the 16x16x32 form exists for the split-list forms of 64-row tiles only");
  constexpr int kT = C::kThreadsW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* tile_buf = smem;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nwg = CRS_NSTREAMS;
  const int qblock = CRS_QBLOCK, stream = CRS_STREAM;
  WP_DECL;
  const bool wave_active = (qblock * (NW * 32) + wave * 32) < a.nq;   // wave-uniform

  // ---- tile transfer (scan_stream.h).  The offsets are lds_dma.h's swizzled_src_offsets written out: through the helper this
  // file's kernels schedule differently (DESIGN.md section 3.1 has the counts)
  unsigned src_off[C::kLoads];
#pragma unroll
  for (int j = 0; j < C::kLoads; ++j) {
    const int P = j * kT + tid;
    const int r = P / C::kCpr, cp = P % C::kCpr;
    src_off[j] = (unsigned)(r * C::kCpr + ((cp & ~15) | ((cp ^ r) & 15))) * 16u;
  }
  const char* slab = reinterpret_cast<const char*>(a.slab);
  const size_t last_chunk = (size_t)a.n_rows * (D * 2) - 16;
  constexpr int RB = C::RB, WTR = C::TR;
  const int n_full = a.n_rows / WTR;
  const unsigned lds_wave = tile_lds_wave(tile_buf, wave);
  auto dma_tile = [&](int tile, int buf) {
    stream_tile<kT, C::kTileBytes>(slab, __builtin_amdgcn_readfirstlane(tile), n_full, last_chunk,
                                   lds_wave + (unsigned)(buf * C::kTileBytes), src_off, wide_streamed<K>() ? a.nt : 0);
  };

  // Tile order: static stride below t_dyn, then (24- / 32-slot forms) ticketed granules -- scan_stream.h, "Tile order"
  __shared__ int sh_next[RING ? 3 : 2];
  constexpr bool kDyn = wide_streamed<K>();
  const int tend = a.n_tiles;
  const int t_dyn = kDyn ? a.t_dyn : a.n_tiles;
  int t = stream, t_prev = stream;
  int tn = t + nwg;     // the look-ahead tile (t_dyn >= 2 nwg: static for the first iteration)
  dma_tile(t, 0);   // goes out before the query fragments are fetched, so the two latencies overlap
  if constexpr (RING) {
    if (tn < tend) dma_tile(tn, 1);   // the ring starts with two tiles landed; a one-tile stream issues nothing past its end
  }

  // ---- this wave's 32 queries, full depth, as B fragments.  32x32x16: lane (n = l & 31, h = l >> 5) holds
  // Q[n][16 ks + 8 h .. + 8] for every k-step ks < D / 16.  16x16x32: two column groups g of 16 queries; lane (n = l & 15,
  // kq = l >> 4) holds Q[16 g + n][32 ks + 8 kq .. + 8] for both groups and every k-step ks < D / 32, group g at qf[g * D/32 + ks]
  // -- the same D / 4 registers.  The query whose LIST the lane keeps (qi) is query n of the wave in the lane pair (l, l ^ 32),
  // resp. query 16 (kq >> 1) + n in the lane pair (l, l ^ 16); h is the lane's half of that pair.
  constexpr int KS16 = D / 32;
  const int kq = lane >> 4;
  const int qn = S16 ? (lane & 15) : (lane & 31), h = S16 ? (kq & 1) : (lane >> 5);
  const int qi = qblock * (NW * 32) + wave * 32 + (S16 ? 16 * (kq >> 1) : 0) + qn;
  const bool q_valid = qi < a.nq;
  f16x8 qf[C::kKsteps];
  {
    // Fetched straight into this layout a load instruction touches 32 rows x 2 pieces of 16 bytes -- 64 cache
    // lines per instruction, D/16 instructions per wave: 12 k cycles of the texture addresser per workgroup,
    // 42 % of a 128-query launch over 100 k rows (tools/scan_wide_probe).  So the wave's 32 query rows come in
    // as whole 128-byte column blocks (8 lanes per row), pass through a wave-private 4 KB of the still idle
    // SECOND (ring form: third) tile buffer (chunk XOR-swizzled by (row >> 1) & 7) and are read back as fragments.  LDS operations of a
    // wave execute in order, so the block's reads see its writes and the next block's writes come after them.
    constexpr int kBlocks = C::kCpr / 8;   // 128-byte column blocks of a query row
    constexpr int kGroup = 3;              // blocks whose loads are in flight together (12 x 16 bytes per lane)
    char* qs = tile_buf + (RING ? 2 : 1) * C::kTileBytes + wave * 4096;
    const int q0 = qblock * (NW * 32) + wave * 32;
    const char* qbytes = reinterpret_cast<const char*>(a.q);
    const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int g0 = 0; g0 < kBlocks; g0 += kGroup) {
      u32x4 tmp[kGroup * 4];
#pragma unroll
      for (int p = 0; p < kGroup; ++p) {
        if (g0 + p < kBlocks) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int c = j * 64 + lane, q = c >> 3, col = c & 7;
            const int qq = q0 + q < a.nq ? q0 + q : a.nq - 1;
            tmp[p * 4 + j] = *reinterpret_cast<const u32x4*>(qbytes + (size_t)qq * (D * 2) + (g0 + p) * 128 + col * 16);
          }
        }
      }
#pragma unroll
      for (int p = 0; p < kGroup; ++p) {
        if (g0 + p < kBlocks) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int c = j * 64 + lane, q = c >> 3, col = c & 7;
            *reinterpret_cast<u32x4*>(qs + q * 128 + ((col ^ ((q >> 1) & 7)) * 16)) = tmp[p * 4 + j];
          }
          if constexpr (S16) {   // chunk 4 kk + kq of the block, rows n and 16 + n; a group's fragments are zero from its first query past nq
#pragma unroll
            for (int g = 0; g < 2; ++g) {
              const int row = 16 * g + qn;
#pragma unroll
              for (int kk = 0; kk < 2; ++kk) {
                const int col = 4 * kk + kq;
                const f16x8 v = *reinterpret_cast<const f16x8*>(qs + row * 128 + ((col ^ ((row >> 1) & 7)) * 16));
                qf[g * KS16 + (g0 + p) * 2 + kk] = (q0 + row < a.nq) ? v : z;
              }
            }
          } else {
#pragma unroll
            for (int ksl = 0; ksl < 4; ++ksl) {
              const int col = 2 * ksl + h;
              const f16x8 v = *reinterpret_cast<const f16x8*>(qs + qn * 128 + ((col ^ ((qn >> 1) & 7)) * 16));
              qf[(g0 + p) * 4 + ksl] = q_valid ? v : z;
            }
          }
        }
      }
    }
#pragma unroll
    for (int ks = 0; ks < C::kKsteps; ++ks) {   // retire these loads here, not somewhere in the loop
      f16x8 x = qf[ks];
      asm volatile("" : "+v"(x));
      qf[ks] = x;
    }
  }
  // A fragment of k-step ks: row (l & 31) of the tile, 16-byte chunk 2 ks + h, through the swizzle; 16x16x32 (as scan_tb.hip):
  // row 16 rt + (l & 15) of the tile's four 16-row blocks, chunk 4 ks + kq
  int a_off[S16 ? 4 : 8];
#pragma unroll
  for (int j = 0; j < (S16 ? 4 : 8); ++j) a_off[j] = qn * (C::kCpr * 16) + ((((S16 ? 4 * j + kq : 2 * j + h)) ^ qn) & 15) * 16;

  // this lane's KL best tiles so far as (best score, first row), sorted by score; split forms: this half's KL ranks of the pair's list
  constexpr bool kSplit = wide_split<K>();
  constexpr int KL = wide_lane_slots<K>();
  float ts[KL];
  int tr[KL];
#pragma unroll
  for (int j = 0; j < KL; ++j) { ts[j] = kNegInf; tr[j] = -1; }

  float px = kNegInf;   // pending candidate of this lane (parity forms; see the loop)
  int pr = -1;

  // split forms: (v, vr) goes in front of the first slot that x does NOT beat, and every slot x beats moves down one place (v is x
  // itself, or in the upper half the slot the lower half pushes out, which x beats too); the compares do not depend on each other
  auto insert_shift = [&](float x, float v, int vr) {
#pragma unroll
    for (int j = 0; j < KL; ++j) {   // (v, vr) is what moves into the next slot x beats: the new entry, then each slot's old content
      const bool c = x > ts[j];
      const float s_old = ts[j];
      const int r_old = tr[j];
      ts[j] = c ? v : s_old;
      tr[j] = c ? vr : r_old;
      v = c ? s_old : v;
      vr = c ? r_old : vr;
    }
  };
  // split forms: one tile's (x, xr) into the pair's list (header: "Split list").  The lower half's last slot as it stands crosses
  // to the upper half: the low-half / even-row value of v_permlane32_swap / v_permlane16_swap, in both lanes of the pair.
  auto pair_bcast = [&](unsigned v, int half) {
    if constexpr (S16) return __builtin_amdgcn_permlane16_swap(v, v, false, false)[half];
    else return __builtin_amdgcn_permlane32_swap(v, v, false, false)[half];
  };
  auto pair_insert = [&](float x, int xr) {
    const float ps = __uint_as_float(pair_bcast(__float_as_uint(ts[KL - 1]), 0));
    const int prow = (int)pair_bcast((unsigned)tr[KL - 1], 0);
    const bool c = h && x > ps;                   // upper half: what the lower half pushes out -- its old last slot, or x itself
    insert_shift(x, c ? ps : x, c ? prow : xr);
  };
  // Deferred insertion (header): the tile waiting for the chain, and a lower bound of the pair's K-th score -- the upper half's last
  // slot as it stood after the last flush, in both lanes of the pair.  (CRS_WIDE_DEFER=0 arrives as a.no_defer: A/B runs)
  constexpr bool kDefer = wide_defer<D, NW, K, S16>();
  const bool defer = kDefer && !a.no_defer;       // a kernel argument: wave-uniform
  float pend_s = kNegInf, thr = kNegInf;
  int pend_r = -1;
  auto flush = [&]() {
    WP_COUNT(5);
    pair_insert(pend_s, pend_r);                  // an empty slot inserts (-inf, -1): beats nothing, moves nothing
    thr = __uint_as_float(pair_bcast(__float_as_uint(ts[KL - 1]), 1));
    pend_s = kNegInf;
    pend_r = -1;
  };
  // One chain site serves both settings of the knob -- with a second one the compiler kept the list in other registers on that path
  // and copied all 2 KL of them over and back on EVERY tile, flush or not.  Knob off: the tile itself is the pending entry and the
  // chain runs at once, which is the undeferred order.
  auto pair_tile = [&](float x, int xr) {
    if constexpr (kDefer) {
      pend_s = defer ? pend_s : x;
      pend_r = defer ? pend_r : xr;
      // strict, as the chain's compares: an equal later tile never enters, nor does a NaN
      const bool run = !defer || __builtin_amdgcn_ballot_w64(x > thr && pend_r >= 0) != 0;
      if (run) flush();                           // some lane's slot is taken: the chain runs, for the whole wave
      const bool cand = defer && x > thr;         // against the refreshed bound
      pend_s = cand ? x : pend_s;
      pend_r = cand ? xr : pend_r;
    } else {
      pair_insert(x, xr);
    }
  };

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();   // the first tile has landed (ring form: the first two), and every wave has its fragments: the last buffer is free
  WP_LAP(0);   // prologue

  // Stagger (MI355X_MICROARCH.md, "two waves per SIMD", item 9).  Waves w and w + 4 share a SIMD, and with
  // one barrier per tile they run in lockstep: both in their MFMA sweep (halving each other's rate), then
  // both in the VALU selection with the matrix pipe idle -- measured 3.7 k cycles per tile against 1.5 k
  // of MFMA work.  So waves 4..7 defer the selection of a tile by one iteration (its 16 accumulators stay
  // in registers across the barrier): on every SIMD one wave multiplies while the other selects.
  // (split forms: CRS_WIDE_STAGGER=0 arrives as a.no_stagger, a kernel argument -- A/B runs; the lists do not depend on it)
  const bool late = wide_stagger<D, NW, K>() && wave >= 4 && !(kSplit && a.no_stagger);   // wave-uniform; off where the deferred accumulators would spill
  using Acc = WAcc<RB, S16>;
  auto zero = [&](Acc& acc) {
    if constexpr (S16) {
#pragma unroll
      for (int rt = 0; rt < 2 * RB; ++rt)
#pragma unroll
        for (int g = 0; g < 2; ++g) acc.a[rt][g] = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc.a[rb][r] = 0.f;
    }
  };
  Acc acc_prev;
  zero(acc_prev);
  auto sweep = [&](const char* buf) {
    Acc acc;
    zero(acc);
    if constexpr (S16) {
      // k-step outermost: 2 RB x 2 accumulators in flight, neighbouring MFMAs never depend on each other, and every A fragment
      // feeds two of them (one per query group).  Each accumulator sums its k-steps in ascending order from zero, which is the
      // arithmetic of the tail's re-score (tail_steps.h, tile_rescore_f16): a representative is bit for bit its row's re-score.
      // The fragments of k-step ks + 1 are fetched while those of ks are multiplied (two sets of 2 RB); the group barriers pin
      // that order, one ds_read_b128 in front of each pair of MFMAs -- left to itself the scheduler fetches a dozen fragments
      // ahead and then funnels the rest through one register quad, a read, a full wait and two MFMAs at a time.
      auto frag = [&](int ks, int rt) {
        return *reinterpret_cast<const f16x8*>(buf + rt * 16 * (C::kCpr * 16) + a_off[ks & 3] + (ks >> 2) * 256);
      };
      f16x8 af[2][2 * RB];
#pragma unroll
      for (int rt = 0; rt < 2 * RB; ++rt) af[0][rt] = frag(0, rt);
      __builtin_amdgcn_sched_group_barrier(0x100, 2 * RB, 0);   // the first set's reads
#pragma unroll
      for (int ks = 0; ks < KS16; ++ks) {
#pragma unroll
        for (int rt = 0; rt < 2 * RB; ++rt) {
          if (ks + 1 < KS16) af[(ks + 1) & 1][rt] = frag(ks + 1, rt);
          acc.a[rt][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[ks & 1][rt], qf[ks], acc.a[rt][0], 0, 0, 0);
          acc.a[rt][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[ks & 1][rt], qf[KS16 + ks], acc.a[rt][1], 0, 0, 0);
          if (ks + 1 < KS16) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // one LDS read
          __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);                      // two MFMAs
        }
      }
    } else {
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
        for (int ks = 0; ks < C::kKsteps; ++ks) {
          const f16x8 af = *reinterpret_cast<const f16x8*>(buf + rb * 32 * (C::kCpr * 16) + a_off[ks & 7] + (ks >> 3) * 256);
          acc.a[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, qf[ks], acc.a[rb], 0, 0, 0);
        }
      }
    }
    return acc;
  };
  // tile te (the ie-th of this stream): the tile's best score for this lane's query -> sorted list.
  // The representative is (best score, first row of the tile): tiles are contiguous row ranges, so on
  // equal scores the lower tile holds the lower rows and no arg-max is needed (scan_refine.hip).
  auto select = [&](const Acc& accs, int te, int ie) {
    float x = kNegInf;
    if constexpr (S16) {
      // lane (n, kq) holds rows 16 rt + 4 kq + i of the tile for queries n (group 0) and 16 + n (group 1)
      float xg[2] = {kNegInf, kNegInf};
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        if (te < n_full) {
          float m[2 * RB];
#pragma unroll
          for (int rt = 0; rt < 2 * RB; ++rt) {
            const f32x4& c = accs.a[rt][g];
            m[rt] = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(c[0], c[1]), c[2]), c[3]);
          }
#pragma unroll
          for (int rt = 0; rt < 2 * RB; rt += 2) xg[g] = __builtin_fmaxf(__builtin_fmaxf(xg[g], m[rt]), m[rt + 1]);
        } else {   // ragged last tile: rows past the end must not win
#pragma unroll
          for (int rt = 0; rt < 2 * RB; ++rt) {
            const int row0 = te * WTR + 16 * rt + 4 * kq;
#pragma unroll
            for (int i = 0; i < 4; ++i) xg[g] = (row0 + i < a.n_rows) ? __builtin_fmaxf(xg[g], accs.a[rt][g][i]) : xg[g];
          }
        }
      }
      // The lane quad of column n serves both queries: lanes kq = 0, 1 keep the list of group 0's, lanes 2, 3 of group 1's.
      // Per group the max over (l, l ^ 16) in all four lanes, then ONE half exchange hands each half of the wave the other half's
      // value of the group it keeps: lanes 32 .. 63 of y0 <-> lanes 0 .. 31 of y1.  (a quad_max per group, one swap less)
      const auto r0 = __builtin_amdgcn_permlane16_swap(__float_as_uint(xg[0]), __float_as_uint(xg[0]), false, false);
      const auto r1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(xg[1]), __float_as_uint(xg[1]), false, false);
      const float y0 = __builtin_fmaxf(__uint_as_float(r0[0]), __uint_as_float(r0[1]));
      const float y1 = __builtin_fmaxf(__uint_as_float(r1[0]), __uint_as_float(r1[1]));
      const auto rr = __builtin_amdgcn_permlane32_swap(__float_as_uint(y0), __float_as_uint(y1), false, false);
      x = __builtin_fmaxf(__uint_as_float(rr[0]), __uint_as_float(rr[1]));   // all four rows of lanes: the tile's best for the lane's query
      pair_tile(x, te * WTR);                       // the pair is (l, l ^ 16)
    } else {   // 32x32x16
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        const f32x16& acc = accs.a[rb];
        if (te < n_full) {
          const float m0 = __builtin_fmaxf(__builtin_fmaxf(acc[0], acc[1]), acc[2]);
          const float m1 = __builtin_fmaxf(__builtin_fmaxf(acc[3], acc[4]), acc[5]);
          const float m2 = __builtin_fmaxf(__builtin_fmaxf(acc[6], acc[7]), acc[8]);
          const float m3 = __builtin_fmaxf(__builtin_fmaxf(acc[9], acc[10]), acc[11]);
          const float m4 = __builtin_fmaxf(__builtin_fmaxf(acc[12], acc[13]), acc[14]);
          x = __builtin_fmaxf(x, __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(m0, m1), __builtin_fmaxf(m2, m3)), __builtin_fmaxf(m4, acc[15])));
        } else {   // ragged last tile: rows past the end must not win
          const int row_base = te * WTR + rb * 32 + 4 * h;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = row_base + 8 * (r >> 2) + (r & 3);
            x = (row < a.n_rows) ? __builtin_fmaxf(x, acc[r]) : x;
          }
        }
      }
      x = pair_max(x);                              // both halves: the tile's best
      if constexpr (kSplit) {
        pair_tile(x, te * WTR);                     // the pair is (l, l ^ 32)
      } else {
        if ((ie & 1) == h) { px = x; pr = te * WTR; } // lane half h is responsible for the tiles of parity h
        if (ie & 1) {
          chain_insert(ts, tr, px, pr);
          px = kNegInf;
          pr = -1;
        }
      }
    }
  };

  int cur = 0, it = 0;
  if constexpr (RING) {
    // one iteration: tile t sits in buffer `cur` of three, tn has landed or is landing in the next one, and the transfer of tnn
    // goes out during the iteration into the one after that (header: "Ring form")
    int tnn = tn + nwg;   // t_dyn >= 3 nwg: static, like tn
    while (t < tend) {
      const bool has_nn = tnn < tend;
      const int nbuf = cur ? cur - 1 : 2;   // (cur + 2) mod 3: last read in the iteration before this one
      const bool in_dyn = tnn >= t_dyn;
      const bool draw = a.ticket != nullptr && has_nn && ticket_due(in_dyn, tnn, nwg, t_dyn, a.dyn_mask);
      // The ticket in flight.  Wave 0 draws, and wave 0 is never idle nor late, so the wait of that path alone names tk and the
      // drawing thread publishes right there: named by the other paths' waits too, tk reached them through a copy made AHEAD of the wait.
      unsigned tk = 0;
      ticket_draw(tk, draw && wave == 0, a.ticket);
      // behind a wave's vmcnt(0) its share of tn has landed; then its share of tnn goes out and stays in flight across the barrier
      auto issue = [&]() {
        WP_LAP(6);   // wait for the next tile (and for the ticket)
        if (has_nn) dma_tile(tnn, nbuf);
        WP_LAP(1);   // tile-load issue
      };
      const char* buf = tile_buf + cur * C::kTileBytes;
      if (!wave_active) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        issue();
      } else if (!late) {   // waves 0..3: the issue falls into what is barrier wait in the two-buffer loop
        const Acc acc = sweep(buf);
        WP_LAP(3);   // MFMA sweep
        select(acc, t, it);
        WP_LAP(4);   // selection (waves 0..3)
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(tk) : : "memory");
        issue();
        if (draw && tid == 0) ticket_publish_slot(sh_next, cur, tk, t_dyn, a.dyn_mask);
      } else {              // waves 4..7: held in issue while the SIMD's other wave multiplies
        if (it > 0) select(acc_prev, t_prev, it - 1);
        WP_LAP(2);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        issue();
        acc_prev = sweep(buf);
        WP_LAP(3);
      }
      int t3 = in_dyn ? tnn + 1 : tnn + nwg;
      // LDS reads and the published ticket only: a vmcnt(0) here (__syncthreads()'s fence has one) would drain the transfer of tnn
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      WP_LAP(7);   // barrier
      if (draw) t3 = ticket_take_slot(sh_next, cur, tend);
      cur = cur == 2 ? 0 : cur + 1;
      ++it;
      t_prev = t;
      t = tn;
      tn = tnn;
      tnn = t3;
    }
    // tiles come in increasing order, so the last two iterations issued nothing: no transfer is in flight (the wait is a guard)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
  // one iteration: tile t sits in LDS buffer `cur`, the look-ahead tile tn streams into the other one
  while (t < tend) {
    const bool has_next = tn < tend;
    if (has_next) dma_tile(tn, cur ^ 1);
    const bool in_dyn = kDyn && tn >= t_dyn;
    const bool draw = kDyn && a.ticket != nullptr && has_next && ticket_due(in_dyn, tn, nwg, t_dyn, a.dyn_mask);
    unsigned tk = 0;   // the ticket in flight: first read behind the vmcnt(0) below
    if constexpr (kDyn) ticket_draw(tk, draw && wave == 0, a.ticket);
    if (wave_active) {
      WP_LAP(1);   // tile-load issue
      const char* buf = tile_buf + cur * C::kTileBytes;
      if (!late) {
        const Acc acc = sweep(buf);
        WP_LAP(3);   // MFMA sweep
        select(acc, t, it);
      } else {       // waves 4..7: last tile's selection first, then this tile's MFMAs
        if (it > 0) select(acc_prev, t_prev, it - 1);
        WP_LAP(2);
        acc_prev = sweep(buf);
        WP_LAP(3);
      }
    }
    WP_LAP(4);   // selection (waves 0..3)
    int tnn = in_dyn ? tn + 1 : tn + nwg;
    if constexpr (kDyn) {
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(tk) : : "memory");
      if (draw && tid == 0) ticket_publish(sh_next, it, tk, t_dyn, a.dyn_mask);
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    WP_LAP(6);   // wait for the next tile (and for the ticket)
    __syncthreads();
    WP_LAP(7);   // barrier
    if (kDyn && draw) tnn = ticket_take(sh_next, it, tend);
    cur ^= 1;
    ++it;
    t_prev = t;
    t = tn;
    tn = tnn;
  }
  }

  if (wave_active && late && it > 0) select(acc_prev, t_prev, it - 1);   // the deferred last tile
  if constexpr (kSplit) {
    if constexpr (kDefer) {
      if (wave_active) flush();   // what still waits for the chain
    }
    if (wave_active && q_valid) {   // [nq, nwg, kp = 2 K]: ranks h KL .. h KL + KL - 1 of the pair's list, then K empty slots
      const size_t o = ((size_t)qi * nwg + stream) * a.kp + (size_t)h * KL;
#pragma unroll
      for (int j = 0; j < KL; ++j) {
        a.part_scores[o + j] = ts[j];
        a.part_rows[o + j] = tr[j];
        a.part_scores[o + K + j] = kNegInf;
        a.part_rows[o + K + j] = -1;
      }
    }
  } else {
    if (wave_active && (it & 1)) chain_insert(ts, tr, px, pr);   // odd tile count: the last (even) tile is still pending
    if (wave_active && q_valid) {   // [nq, nwg, kp = 2 K]: lane half h owns slots h K .. h K + K - 1
      const size_t o = ((size_t)qi * nwg + stream) * a.kp + (size_t)h * K;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        a.part_scores[o + j] = ts[j];
        a.part_rows[o + j] = tr[j];
      }
    }
  }
  WP_LAP(10);   // final flush
  WP_STORE(NW);
}

// Which kernels a translation unit holds: 0 (scan_wide.hip itself) the two-buffer kernels of every form, 1 (scan_wide_ring.hip) the
// ring kernels, 2 (tools/scan_wide_probe.hip) both
#ifndef CRS_WIDE_TU
#define CRS_WIDE_TU 0
#endif

#if CRS_WIDE_TU != 1
template <int D, int NW, int K>
__global__ __launch_bounds__(NW * 64, 2) void scan_wide_kernel(const ScanArgs a) {
  scan_wide_body<D, NW, K, false>(a);
}
// the 16x16x32 form of the same launch: same grid, same LDS, same partial lists
template <int D, int NW, int K>
__global__ __launch_bounds__(NW * 64, 2) void scan_wide16_kernel(const ScanArgs a) {
  scan_wide_body<D, NW, K, true>(a);
}

template <int D, int NW, int K, bool S16>
int launch_wide(const ScanArgs& a, hipStream_t stream) {
  if constexpr (S16) return launch_scan<&scan_wide16_kernel<D, NW, K>>(WCfg<D, NW>::kLds, NW * 64, a, stream);
  else return launch_scan<&scan_wide_kernel<D, NW, K>>(WCfg<D, NW>::kLds, NW * 64, a, stream);
}

// the form if scan_forms.h has it
template <int D, int NW, int K>
int launch_wide_if(const ScanArgs& a, int mfma, hipStream_t stream) {
  if constexpr (wide_form_exists(D, NW, K, 16)) {
    if (mfma == 16) return launch_wide<D, NW, K, true>(a, stream);
  }
  if constexpr (wide_form_exists(D, NW, K, 32)) return launch_wide<D, NW, K, false>(a, stream);
  else return -1;
}

template <int D, int NW>
int launch_wide_k(const ScanArgs& a, int mfma, hipStream_t stream) {
  switch (scan_wide_slots(a.k)) {
    case 4: return launch_wide_if<D, NW, 4>(a, mfma, stream);
    case 10: return launch_wide_if<D, NW, 10>(a, mfma, stream);
    case 16: return launch_wide_if<D, NW, 16>(a, mfma, stream);
    case 24: return launch_wide_if<D, NW, 24>(a, mfma, stream);
    default: return launch_wide_if<D, NW, 32>(a, mfma, stream);
  }
}

template <int D>
int launch_wide_d(const ScanArgs& a, int nw, int mfma, hipStream_t stream) {
  return nw == 8 ? launch_wide_k<D, 8>(a, mfma, stream) : launch_wide_k<D, 4>(a, mfma, stream);
}

#endif   // CRS_WIDE_TU != 1

#if CRS_WIDE_TU != 0
// The ring kernels of the forms of wide_ring<>: same grid and partial lists, three tile buffers of LDS.  They carry their form's
// kernel names inside a namespace of their own, so a launch trace keeps naming the form: ring::scan_wide16_kernel<384, 8, 24>.
namespace ring {
template <int D, int NW, int K>
__global__ __launch_bounds__(NW * 64, 2) void scan_wide_kernel(const ScanArgs a) {
  scan_wide_body<D, NW, K, false, true>(a);
}
template <int D, int NW, int K>
__global__ __launch_bounds__(NW * 64, 2) void scan_wide16_kernel(const ScanArgs a) {
  scan_wide_body<D, NW, K, true, true>(a);
}
}  // namespace ring

template <int D, int K>
int launch_ring_if(const ScanArgs& a, int mfma, hipStream_t stream) {
  if constexpr (wide_ring<D, 8, K, true>()) {
    if (mfma == 16) return launch_scan<&ring::scan_wide16_kernel<D, 8, K>>(WCfg<D, 8>::kLdsRing, 8 * 64, a, stream);
  }
  if constexpr (wide_ring<D, 8, K, false>()) {
    if (mfma == 32) return launch_scan<&ring::scan_wide_kernel<D, 8, K>>(WCfg<D, 8>::kLdsRing, 8 * 64, a, stream);
  }
  return -1;
}

template <int D>
int launch_ring_d(const ScanArgs& a, int mfma, hipStream_t stream) {
  switch (scan_wide_slots(a.k)) {
    case 24: return launch_ring_if<D, 24>(a, mfma, stream);
    case 32: return launch_ring_if<D, 32>(a, mfma, stream);
    default: return -1;
  }
}
#endif   // CRS_WIDE_TU != 0

}  // namespace

#if CRS_WIDE_TU != 1
int scan_launch_wide(const ScanArgs& a, int pdim, int nw, int mfma, hipStream_t stream) {
  switch (pdim) {
    case 128: return launch_wide_d<128>(a, nw, mfma, stream);
    case 256: return launch_wide_d<256>(a, nw, mfma, stream);
    case 384: return launch_wide_d<384>(a, nw, mfma, stream);
    case 512: return launch_wide_d<512>(a, nw, mfma, stream);
    default: return -1;
  }
}
#endif

#if CRS_WIDE_TU != 0
int scan_launch_wide_ring(const ScanArgs& a, int pdim, int nw, int mfma, hipStream_t stream) {
  if (nw != 8) return -1;
  switch (pdim) {
    case 128: return launch_ring_d<128>(a, mfma, stream);
    case 256: return launch_ring_d<256>(a, mfma, stream);
    case 384: return launch_ring_d<384>(a, mfma, stream);
    default: return -1;
  }
}
#endif

}  // namespace crs
