// unigram.hip -- SentencePiece Unigram tokenisation on the device (gfx950): crs_unigram_encode.  UTF-8 texts in, <s> ids </s> pad
// rows out: what the `tokenizers` library computes for XLM-RoBERTa's pipeline (normaliser, Replace(" {2,}"), WhitespaceSplit +
// Metaspace, Unigram, TemplateProcessing single).  rag/_unigram.py builds the tables and restates this file in Python.
//
// One workgroup of 256 threads per text, the text walked in tiles of kTile bytes, as in wordpiece.hip:
//   1. the tile's bytes (+ 3 of look-ahead) are staged in LDS;
//   2. each lane decodes the code points whose lead byte lies in its 4 bytes, looks each up in the normalisation table and emits
//      0-3 RAW elements: a normalised code point with a kind (character, U+0020, other white space, U+2581).  A block scan
//      compacts them behind what the previous tile carried over.  CR in front of LF emits nothing when the normaliser joins them;
//   3. every raw element learns its role from its neighbours: a lone U+0020 and a run of two or more (what Replace(" {2,}") sees)
//      either end a word or become one metaspace; a character behind a word end gets the metaspace that Metaspace prepends.  A
//      second scan writes the WORD array: every word opens with U+2581, so a word runs to the next U+2581;
//   4. one lane per word start runs the Viterbi walk of Unigram::encode_optimized on its word: starts ascending, every piece
//      length looked up under a running FNV-1a hash, best[end] replaced only by a strictly greater fp64 sum, an unknown candidate
//      of one character at unk_score where no one-character piece matches; then the back-pointers are walked, unknowns next to
//      each other fusing into one id.  Best sum, piece id and back-pointer sit in LDS arrays parallel to the word array;
//   5. a third scan, over the words' id counts, places the ids in the output row.
// The word that the tile's end cuts is carried to the front of the raw array (metaspace first), be it a lone metaspace; where
// runs of U+0020 collapse (CRS_UNIGRAM_COLLAPSE), a run at the tile's end is carried instead, as one or two elements.  A word of
// more than kMaxWord code points (its metaspace included) flags the text for the host: Unigram has no rule that shortens a word.
// The walk stops once max_len - 2 ids exist.  Every loop is bounded: tiles by the text's length, starts and ends by the word's
// length, lengths by lmax, probes by max_probe.  No atomics on global memory, no workspace; the same input gives the same output.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crs_hip.h"
#include "scan.h"

namespace crs {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = CRS_UNIGRAM_TILE_BYTES;
constexpr int kPerLane = kTile / kThreads;
constexpr int kMaxWord = CRS_UNIGRAM_MAX_WORD;
constexpr int kRaw = kMaxWord + kTile + kTile / 2 + 32;   // carry + 1.5 elements per byte (a 2-byte character -> 3 code points)
constexpr int kFin = kRaw + 1;                            // one prepended metaspace per word end, plus one for the array's front
constexpr int kPerThread = (kFin + kThreads - 1) / kThreads;
static_assert(kTile % kThreads == 0 && kPerLane == 4, "a lane owns 4 bytes of the tile");
static_assert(kMaxWord <= kThreads && kMaxWord < 65535, "the carried word is copied by one lane per element");

// raw element: bits 0-20 code point | bits 29-30 kind
constexpr uint32_t kCpMask = 0x1FFFFF, kKindShift = 29;
constexpr uint32_t kChar = 0, kSp = 1, kBrk = 2, kMeta = 3;
constexpr uint32_t kMetaCp = 0x2581;
constexpr uint32_t kFnvPrime = 16777619u, kSeedWord = 2166136261u;
constexpr uint16_t kUnset = 0xFFFF;

struct Args {
  const uint8_t* text;
  const int64_t* offsets;
  int64_t n_bytes;
  const uint32_t* table;
  int64_t table_len;
  const uint32_t* rep;
  int64_t rep_len;
  const int4* slots;
  const double* slot_scores;
  uint32_t slot_mask;
  const uint32_t* pool;
  int64_t pool_len;
  double unk_score;
  int max_probe, lmax, opts, unk, cls, sep, pad, max_len;
  int* ids;
  int* lens;
  int* flags;
};

// exclusive prefix sum of `v` over the 256 threads; *total = the sum.  `sh` holds 4 ints; two barriers.
__device__ inline int block_scan(int v, int* sh, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  int base = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) {
    const int s = sh[w];
    if (w < wave) base += s;
    sum += s;
  }
  __syncthreads();
  *total = sum;
  return base + inc - v;
}

// slot index of the piece w[0 .. n) with hash h, or -1
__device__ inline int vocab_find(const Args& a, const uint32_t* w, int n, uint32_t h) {
  uint32_t s = (h ^ (h >> 15)) & a.slot_mask;
  for (int p = 0; p < a.max_probe; ++p, s = (s + 1) & a.slot_mask) {
    const int4 slot = a.slots[s];
    if (slot.y == 0) return -1;
    if ((uint32_t)slot.w != h || slot.y != n) continue;
    const int64_t off = (uint32_t)slot.x;
    if (off + n > a.pool_len) continue;
    bool same = true;
    for (int k = 0; k < n; ++k) same = same && a.pool[off + k] == w[k];
    if (same) return (int)s;
  }
  return -1;
}

__device__ inline bool is_sp(uint32_t e) { return (e >> kKindShift) == kSp; }

__global__ __launch_bounds__(kThreads) void unigram_kernel(const Args a) {
  __shared__ uint8_t s_bytes[kTile + 4];
  __shared__ uint32_t s_raw[kFin];      // raw elements (kRaw of them); once the word array is written, the words' ids (s_out)
  __shared__ uint32_t s_fin[kFin];      // the word array: code points, every word opening with U+2581
  __shared__ double s_best[kFin];       // best sum of a path ending behind this element
  __shared__ int s_id[kFin];            // ... its last piece
  __shared__ uint16_t s_back[kFin];     // ... where that piece starts (offset in the word); kUnset: no path yet
  __shared__ uint16_t s_cnt[kFin];      // at a word start: the word's ids
  __shared__ int s_scan[4];
  __shared__ int s_last_nonsp, s_last_start, s_fallback;
  int* const s_out = reinterpret_cast<int*>(s_raw);

  const int tid = threadIdx.x;
  const int row = blockIdx.x;
  int64_t t0 = a.offsets[row], t1 = a.offsets[row + 1];
  t0 = t0 < 0 ? 0 : (t0 > a.n_bytes ? a.n_bytes : t0);
  t1 = t1 < t0 ? t0 : (t1 > a.n_bytes ? a.n_bytes : t1);
  const int64_t n_bytes = t1 - t0;
  const uint8_t* text = a.text + t0;
  const int budget = a.max_len - 2;
  int* out = a.ids + (int64_t)row * a.max_len;
  const bool collapse = a.opts & CRS_UNIGRAM_COLLAPSE, single_meta = a.opts & CRS_UNIGRAM_SINGLE_META,
             run_meta = a.opts & CRS_UNIGRAM_RUN_META, crlf = a.opts & CRS_UNIGRAM_CRLF;

  if (tid == 0) s_fallback = 0;
  __syncthreads();

  int n_tok = 0;     // ids so far (uniform)
  int carry = 0;     // raw elements already at the front of s_raw (uniform)
  bool bad = false;  // s_fallback, read behind a barrier (uniform)
  for (int64_t pos = 0; pos < n_bytes && n_tok < budget && !bad; pos += kTile) {
    const bool last_tile = pos + kTile >= n_bytes;
    // 1. stage
    for (int i = tid; i < kTile + 3; i += kThreads) s_bytes[i] = (pos + i < n_bytes) ? text[pos + i] : 0;
    if (tid == 0) { s_last_nonsp = -1; s_last_start = -1; }
    __syncthreads();

    // 2. decode, look up, emit
    uint32_t ent[kPerLane];
    int n_em = 0;
    bool fallback = false;
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
      const int i = tid * kPerLane + j;
      const uint32_t b0 = s_bytes[i];
      ent[j] = 0;
      if (pos + i >= n_bytes || (b0 & 0xC0) == 0x80) continue;
      uint32_t cp;
      if (b0 < 0x80) cp = b0;
      else if (b0 < 0xE0) cp = ((b0 & 0x1F) << 6) | (s_bytes[i + 1] & 0x3F);
      else if (b0 < 0xF0) cp = ((b0 & 0x0F) << 12) | ((s_bytes[i + 1] & 0x3Fu) << 6) | (s_bytes[i + 2] & 0x3F);
      else cp = ((b0 & 0x07) << 18) | ((s_bytes[i + 1] & 0x3Fu) << 12) | ((s_bytes[i + 2] & 0x3Fu) << 6) | (s_bytes[i + 3] & 0x3F);
      if (crlf && cp == 0x0D && pos + i + 1 < n_bytes && s_bytes[i + 1] == 0x0A) continue;    // CR LF is the LF's one space
      if ((int64_t)cp >= a.table_len) { fallback = true; continue; }
      const uint32_t e = a.table[cp];
      const uint32_t cls = e & 7, n = (e >> 3) & 3;
      if (cls == 4 || (n >= 2 && (int64_t)(e >> 11) + n > a.rep_len)) { fallback = true; continue; }
      if (cls != 3) continue;
      ent[j] = e;
      n_em += (int)n;
    }
    if (fallback) s_fallback = 1;
    int total;
    int at_el = carry + block_scan(n_em, s_scan, &total);
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
      const uint32_t e = ent[j];
      const uint32_t n = (e >> 3) & 3, v = e >> 11;
      for (uint32_t k = 0; k < n; ++k, ++at_el) {
        const uint32_t cp = (n == 1) ? v : a.rep[v + k];
        if (at_el < kRaw) s_raw[at_el] = (cp & kCpMask) | (((e >> (5 + 2 * k)) & 3) << kKindShift);
      }
    }
    int n_raw = carry + total;
    if (n_raw > kRaw) n_raw = kRaw;        // cannot happen with a table from rag/_unigram.py; keeps a malformed one in bounds
    __syncthreads();

    // 3. roles.  Where runs collapse, a run of U+0020 at the tile's end waits for the next tile: its length is not known yet.
    // Where they do not, every U+0020 has its role at once, and holding a run back as two elements would lose the others
    for (int i = tid; i < n_raw; i += kThreads)
      if (!is_sp(s_raw[i])) atomicMax(&s_last_nonsp, i);
    __syncthreads();
    const int n_proc = (last_tile || !collapse) ? n_raw : s_last_nonsp + 1;
    const int tail_sp = n_raw - n_proc;
    // what raw element i puts into the word array: 0, 1 or 2 code points
    auto sp_is_meta = [&](int i) {           // s_raw[i] is U+0020: does its run (or it alone) stand for a metaspace?
      const bool run = collapse && ((i > 0 && is_sp(s_raw[i - 1])) || (i + 1 < n_raw && is_sp(s_raw[i + 1])));
      return run ? run_meta : single_meta;
    };
    auto emits = [&](int i) {
      const uint32_t e = s_raw[i], kind = e >> kKindShift;
      if (kind == kBrk) return 0;
      if (kind == kMeta) return 1;
      if (kind == kSp) {
        if (!sp_is_meta(i)) return 0;
        return (collapse && i > 0 && is_sp(s_raw[i - 1])) ? 0 : 1;      // the run's first element stands for it
      }
      bool after_end;                        // a character: behind a word end it gets the prepended metaspace
      if (i == 0) after_end = carry == 0;
      else {
        const uint32_t pk = s_raw[i - 1] >> kKindShift;
        after_end = pk == kBrk || (pk == kSp && !sp_is_meta(i - 1));
      }
      return after_end ? 2 : 1;
    };
    int mine = 0;
    {
      const int lo = tid * kPerThread, hi = (lo + kPerThread < n_proc) ? lo + kPerThread : n_proc;
      for (int i = lo; i < hi; ++i) mine += emits(i);
    }
    int n_fin;
    int at_f = block_scan(mine, s_scan, &n_fin);
    {
      const int lo = tid * kPerThread, hi = (lo + kPerThread < n_proc) ? lo + kPerThread : n_proc;
      for (int i = lo; i < hi; ++i) {
        const int c = emits(i);
        const uint32_t kind = s_raw[i] >> kKindShift;
        if (c == 2) {
          if (at_f < kFin) s_fin[at_f] = kMetaCp;
          ++at_f;
        }
        if (c >= 1) {
          if (at_f < kFin) s_fin[at_f] = (kind == kChar) ? (s_raw[i] & kCpMask) : kMetaCp;
          ++at_f;
        }
      }
    }
    if (n_fin > kFin) n_fin = kFin;
    const uint32_t sp0 = (tail_sp > 0) ? s_raw[n_proc] : 0;       // the waiting run, read before s_raw becomes s_out
    const uint32_t last_kind = (n_proc > 0) ? s_raw[n_proc - 1] >> kKindShift : kBrk;
    // does the tile's last element leave a word open?  A U+0020 ends a tile that is not the last only where runs do not collapse,
    // and there it opens a word, as U+2581 itself does, when it stands for a metaspace
    const bool open_end = last_kind == kChar || last_kind == kMeta || (last_kind == kSp && single_meta);
    __syncthreads();

    // 4. words
    for (int i = tid; i < n_fin; i += kThreads) {
      const bool start = s_fin[i] == kMetaCp;
      s_cnt[i] = 0;
      if (start) atomicMax(&s_last_start, i);
    }
    __syncthreads();
    const int last_start = s_last_start;
    // the last word is cut by the tile's end unless the text ends here or something behind it ended it
    const bool cut = !last_tile && last_start >= 0 && tail_sp == 0 && open_end;
    for (int i = tid; i < n_fin; i += kThreads) {
      if (s_fin[i] != kMetaCp) continue;
      const uint32_t* w = s_fin + i;
      int len = 1;
      for (; len <= kMaxWord && i + len < n_fin && w[len] != kMetaCp; ++len) {}
      if (len > kMaxWord) { s_fallback = 1; continue; }
      if (cut && i == last_start) continue;
      for (int k = 0; k < len; ++k) s_back[i + k] = kUnset;
      for (int s = 0; s < len; ++s) {
        const double till = s ? s_best[i + s - 1] : 0.0;
        bool single = false;
        uint32_t h = kSeedWord;
        const int lim = (len < s + a.lmax) ? len : s + a.lmax;
        for (int e = s; e < lim; ++e) {
          h = (h ^ w[e]) * kFnvPrime;
          const int slot = vocab_find(a, w + s, e + 1 - s, h);
          if (slot < 0) continue;
          const double cand = a.slot_scores[slot] + till;
          if (s_back[i + e] == kUnset || cand > s_best[i + e]) {
            s_best[i + e] = cand;
            s_id[i + e] = a.slots[slot].z;
            s_back[i + e] = (uint16_t)s;
          }
          if (e == s) single = true;
        }
        if (!single) {
          const double cand = a.unk_score + till;
          if (s_back[i + s] == kUnset || cand > s_best[i + s]) {
            s_best[i + s] = cand;
            s_id[i + s] = a.unk;
            s_back[i + s] = (uint16_t)s;
          }
        }
      }
      // walk back: count, then write from the word's last id to its first
      int n_out = 0;
      bool prev_unk = false;
      for (int e = len, g = 0; e > 0 && g < len; ++g) {
        const bool u = s_id[i + e - 1] == a.unk;
        if (!(u && prev_unk)) ++n_out;
        prev_unk = u;
        const int b = s_back[i + e - 1];
        e = (b < e) ? b : 0;
      }
      prev_unk = false;
      for (int e = len, g = 0, k = n_out; e > 0 && g < len; ++g) {
        const int id = s_id[i + e - 1];
        const bool u = id == a.unk;
        if (!(u && prev_unk) && k > 0) s_out[i + --k] = id;
        prev_unk = u;
        const int b = s_back[i + e - 1];
        e = (b < e) ? b : 0;
      }
      s_cnt[i] = (uint16_t)n_out;
    }
    __syncthreads();
    bad = s_fallback != 0;

    // 5. place the ids
    int ids_mine = 0;
    const int lo = tid * kPerThread, hi = (lo + kPerThread < n_fin) ? lo + kPerThread : n_fin;
    for (int i = lo; i < hi; ++i) ids_mine += s_cnt[i];
    int tile_tok;
    int at = n_tok + block_scan(ids_mine, s_scan, &tile_tok);
    for (int i = lo; i < hi; ++i)
      for (int k = 0, c = s_cnt[i]; k < c; ++k, ++at)
        if (at < budget) out[1 + at] = s_out[i + k];
    n_tok += tile_tok;
    __syncthreads();

    // what waits for the next tile goes to the front of the raw array
    carry = 0;
    if (cut) {
      const int len = n_fin - last_start;        // <= kMaxWord, or the text is flagged and the loop ends
      if (len <= kMaxWord) {
        if (tid < len) s_raw[tid] = s_fin[last_start + tid] | ((tid == 0 ? kMeta : kChar) << kKindShift);
        carry = len;
      }
    } else if (tail_sp > 0) {
      if (tid < 2) s_raw[tid] = sp0;
      carry = tail_sp >= 2 ? 2 : 1;
    }
    __syncthreads();
  }

  if (n_tok > budget) n_tok = budget;
  if (tid == 0) {
    out[0] = a.cls;
    out[1 + n_tok] = a.sep;
    a.lens[row] = n_tok + 2;
    a.flags[row] = s_fallback;
  }
  for (int i = n_tok + 2 + tid; i < a.max_len; i += kThreads) out[i] = a.pad;
}

}  // namespace

int unigram_encode_launch(const uint8_t* text, const int64_t* offsets, int n_texts, int64_t n_bytes, const uint32_t* table,
                          int64_t table_len, const uint32_t* rep, int64_t rep_len, const int32_t* slots, const double* slot_scores,
                          int64_t n_slots, const uint32_t* pool, int64_t pool_len, int max_probe, int lmax, double unk_score, int opts,
                          int unk, int cls, int sep, int pad, int max_len, int* ids, int* lens, int* flags, hipStream_t stream) {
  Args a;
  a.text = text; a.offsets = offsets; a.n_bytes = n_bytes;
  a.table = table; a.table_len = table_len; a.rep = rep; a.rep_len = rep_len;
  a.slots = reinterpret_cast<const int4*>(slots); a.slot_scores = slot_scores; a.slot_mask = (uint32_t)(n_slots - 1);
  a.pool = pool; a.pool_len = pool_len; a.unk_score = unk_score;
  a.max_probe = max_probe; a.lmax = lmax; a.opts = opts; a.unk = unk; a.cls = cls; a.sep = sep; a.pad = pad; a.max_len = max_len;
  a.ids = ids; a.lens = lens; a.flags = flags;
  hipLaunchKernelGGL(unigram_kernel, dim3(n_texts), dim3(kThreads), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace crs
