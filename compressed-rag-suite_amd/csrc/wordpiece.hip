// wordpiece.hip -- BERT tokenisation on the device (gfx950): crs_wordpiece_encode.  UTF-8 texts in, [CLS] ids [SEP] pad rows out.
//
// One workgroup of 256 threads per text.  The text is walked in tiles of kTile bytes:
//   1. the tile's bytes (+ 3 bytes of look-ahead for a character that straddles the tile's end) are staged in LDS;
//   2. each lane decodes the code points whose LEAD byte lies in its 4 bytes, looks each up in the normalisation table (one uint32
//      per code point: rag/_wordpiece.py) and emits 0-3 elements: a normalised code point with a "stands alone" bit (punctuation,
//      CJK), or a separator for white space.  A block prefix scan compacts the elements into an LDS array, behind the unfinished
//      word carried over from the previous tile;
//   3. one lane per word start (elements are dealt round-robin, so the words spread evenly over the lanes) runs WordPiece on its
//      word straight out of that array: the piece grows one code point at a time under a running FNV-1a hash, every length is
//      looked up in the vocabulary hash table, the longest hit wins -- the same piece as trying the longest first.  A position
//      with no hit, or a word of more than 100 code points, makes the word one [UNK].  The word's ids go to a second LDS array,
//      at the word's own position (a word has no more ids than code points);
//   4. a second scan, over the words' id counts, places the ids in the output row.
// The word that the tile's end cuts is not tokenised but moved to the front of the array for the next tile; once it is longer
// than 100 code points only a marker is kept (WordPiece mode), or the CRC so far (hash mode).  The walk stops as soon as
// max_len - 2 ids exist.  Every loop is bounded: tiles by the text's length, pieces by the word's length, lengths by lmax, probes
// by max_probe.  No atomics on global memory, no workspace; the same input gives the same output.
//
// mode 1 is rag.tokenizer.HashTokenizer's rule: one id per word, lo + crc32(UTF-8 of the word) % span (zlib's CRC-32, by table).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crs_hip.h"
#include "scan.h"

namespace crs {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = CRS_WORDPIECE_TILE_BYTES;
constexpr int kPerLane = kTile / kThreads;          // bytes per lane
constexpr int kMaxWord = 100;                       // max_input_chars_per_word
constexpr int kElems = kMaxWord + kTile + kTile / 2 + 28;   // carry + 1.5 elements per byte (a 2-byte character -> 3 code points)
constexpr int kPerThread = (kElems + kThreads - 1) / kThreads;
static_assert(kTile % kThreads == 0 && kPerLane == 4, "a lane owns 4 bytes of the tile");

// element: bits 0-20 code point | kAlone | kSep | kMark
constexpr uint32_t kAlone = 1u << 29;   // a word of its own
constexpr uint32_t kSep = 1u << 30;     // white space
constexpr uint32_t kMark = 1u << 31;    // stands for the carried part of a word that is not kept as characters
constexpr uint32_t kCpMask = 0x1FFFFF;

constexpr uint32_t kFnvPrime = 16777619u, kSeedWord = 2166136261u, kSeedCont = 2166136261u ^ 0x9E3779B9u;

struct Crc32Table {
  uint32_t v[256];
  constexpr Crc32Table() : v() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
      v[i] = c;
    }
  }
};
__device__ const Crc32Table g_crc32 = Crc32Table();

struct Args {
  const uint8_t* text;
  const int64_t* offsets;
  int64_t n_bytes;
  const uint32_t* table;
  int64_t table_len;
  const uint32_t* rep;
  int64_t rep_len;
  const int4* slots;
  uint32_t slot_mask;
  const uint32_t* pool;
  int64_t pool_len;
  int max_probe, lmax, mode, unk, cls, sep, pad, hash_lo, hash_span, max_len;
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

__device__ inline uint32_t crc_byte(const uint32_t* crc_tab, uint32_t crc, uint32_t b) { return crc_tab[(crc ^ b) & 255] ^ (crc >> 8); }

// the CRC-32 state after the UTF-8 bytes of code point cp
__device__ inline uint32_t crc_cp(const uint32_t* crc_tab, uint32_t crc, uint32_t cp) {
  if (cp < 0x80) return crc_byte(crc_tab, crc, cp);
  if (cp < 0x800) {
    crc = crc_byte(crc_tab, crc, 0xC0 | (cp >> 6));
    return crc_byte(crc_tab, crc, 0x80 | (cp & 63));
  }
  if (cp < 0x10000) {
    crc = crc_byte(crc_tab, crc, 0xE0 | (cp >> 12));
    crc = crc_byte(crc_tab, crc, 0x80 | ((cp >> 6) & 63));
    return crc_byte(crc_tab, crc, 0x80 | (cp & 63));
  }
  crc = crc_byte(crc_tab, crc, 0xF0 | (cp >> 18));
  crc = crc_byte(crc_tab, crc, 0x80 | ((cp >> 12) & 63));
  crc = crc_byte(crc_tab, crc, 0x80 | ((cp >> 6) & 63));
  return crc_byte(crc_tab, crc, 0x80 | (cp & 63));
}

// id of the piece elems[0 .. n) (continuation: `cont`) with hash h, or -1
__device__ inline int vocab_find(const Args& a, const uint32_t* elems, int n, uint32_t cont, uint32_t h) {
  const uint32_t tag = (uint32_t)n | (cont << 31);
  uint32_t s = (h ^ (h >> 15)) & a.slot_mask;
  for (int p = 0; p < a.max_probe; ++p, s = (s + 1) & a.slot_mask) {
    const int4 slot = a.slots[s];
    if (slot.y == 0) return -1;
    if ((uint32_t)slot.w != h || (uint32_t)slot.y != tag) continue;
    const int64_t off = (uint32_t)slot.x;
    if (off + n > a.pool_len) continue;
    bool same = true;
    for (int k = 0; k < n; ++k) same = same && a.pool[off + k] == (elems[k] & kCpMask);
    if (same) return slot.z;
  }
  return -1;
}

__global__ __launch_bounds__(kThreads) void wordpiece_kernel(const Args a) {
  __shared__ uint8_t s_bytes[kTile + 4];
  __shared__ uint32_t s_elems[kElems];
  __shared__ int s_tok[kElems];
  __shared__ uint16_t s_cnt[kElems];
  __shared__ uint32_t s_crc[256];
  __shared__ int s_scan[4];
  __shared__ int s_last_start;      // index of the last word start of the tile's array
  __shared__ uint32_t s_carry_crc[2];  // hash mode: the CRC state of the carried word; read [tile & 1], written [~tile & 1]
  __shared__ int s_fallback;

  const int tid = threadIdx.x;
  const int row = blockIdx.x;
  int64_t t0 = a.offsets[row], t1 = a.offsets[row + 1];
  t0 = t0 < 0 ? 0 : (t0 > a.n_bytes ? a.n_bytes : t0);
  t1 = t1 < t0 ? t0 : (t1 > a.n_bytes ? a.n_bytes : t1);
  const int64_t n_bytes = t1 - t0;
  const uint8_t* text = a.text + t0;
  const int budget = a.max_len - 2;
  int* out = a.ids + (int64_t)row * a.max_len;

  s_crc[tid] = g_crc32.v[tid];
  if (tid == 0) { s_fallback = 0; s_carry_crc[0] = s_carry_crc[1] = 0; }
  __syncthreads();

  int n_tok = 0;     // ids so far (uniform)
  int carry = 0;     // elements already at the front of s_elems (uniform)
  int par = 0;       // tile parity
  for (int64_t pos = 0; pos < n_bytes && n_tok < budget; pos += kTile, par ^= 1) {
    const bool last_tile = pos + kTile >= n_bytes;
    // 1. stage
    for (int i = tid; i < kTile + 3; i += kThreads) s_bytes[i] = (pos + i < n_bytes) ? text[pos + i] : 0;
    if (tid == 0) s_last_start = -1;
    __syncthreads();

    // 2. decode, look up, emit
    uint32_t ent[kPerLane];     // the table entries of this lane's characters; 0 (class DROP, nothing emitted) where there is none
    int n_em = 0;
    bool fallback = false;
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
      const int i = tid * kPerLane + j;
      const uint32_t b0 = s_bytes[i];
      ent[j] = 0;
      if (pos + i >= n_bytes || (b0 & 0xC0) == 0x80) continue;     // past the end, or not a lead byte
      uint32_t cp;
      if (b0 < 0x80) cp = b0;
      else if (b0 < 0xE0) cp = ((b0 & 0x1F) << 6) | (s_bytes[i + 1] & 0x3F);
      else if (b0 < 0xF0) cp = ((b0 & 0x0F) << 12) | ((s_bytes[i + 1] & 0x3Fu) << 6) | (s_bytes[i + 2] & 0x3F);
      else cp = ((b0 & 0x07) << 18) | ((s_bytes[i + 1] & 0x3Fu) << 12) | ((s_bytes[i + 2] & 0x3Fu) << 6) | (s_bytes[i + 3] & 0x3F);
      if ((int64_t)cp >= a.table_len) { fallback = true; continue; }
      const uint32_t e = a.table[cp];
      const uint32_t cls = e & 7, n = (e >> 3) & 3;
      if (cls >= 4 || (n >= 2 && (int64_t)(e >> 8) + n > a.rep_len)) { fallback = true; continue; }
      ent[j] = e;
      n_em += (cls == 1) ? 1 : (int)n;
    }
    if (fallback) s_fallback = 1;
    int total;
    int at_el = carry + block_scan(n_em, s_scan, &total);
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
      const uint32_t e = ent[j];
      const uint32_t cls = e & 7, n = (e >> 3) & 3, v = e >> 8;
      const uint32_t alone_all = (cls == 2) ? kAlone : 0;
      if (cls == 1) {
        if (at_el < kElems) s_elems[at_el] = kSep;
        ++at_el;
      } else if (n == 1) {
        if (at_el < kElems) s_elems[at_el] = (v & kCpMask) | (((e >> 5) & 1) ? kAlone : alone_all);
        ++at_el;
      } else {
        for (uint32_t k = 0; k < n; ++k, ++at_el)
          if (at_el < kElems) s_elems[at_el] = (a.rep[v + k] & kCpMask) | (((e >> (5 + k)) & 1) ? kAlone : alone_all);
      }
    }
    int n_el = carry + total;
    if (n_el > kElems) n_el = kElems;      // cannot happen with a table from rag/_wordpiece.py; keeps a malformed one in bounds
    __syncthreads();

    // 3. words: which elements start one, and which start is the last
    for (int i = tid; i < n_el; i += kThreads) {
      const uint32_t e = s_elems[i];
      bool start = !(e & kSep);
      if (start && i > 0) {
        const uint32_t p = s_elems[i - 1];
        start = (p & (kSep | kAlone)) || (e & kAlone);
      }
      s_cnt[i] = start ? 1 : 0;
      if (start) atomicMax(&s_last_start, i);
    }
    __syncthreads();
    // the word at the last start is cut by the tile's end unless the text ends here or the array ends in a separator / lone element
    const int last_start = s_last_start;
    const bool cut = !last_tile && last_start >= 0 && !(s_elems[n_el - 1] & (kSep | kAlone));
    for (int i = tid; i < n_el; i += kThreads) {
      if (!s_cnt[i]) continue;
      if (cut && i == last_start && a.mode == 0) { s_cnt[i] = 0; continue; }      // carried as characters (or as the marker) below
      const uint32_t* w = s_elems + i;
      const bool marked = (w[0] & kMark) != 0;
      if (a.mode == 1) {                   // hash mode: CRC of the whole word, however long
        uint32_t crc = marked ? s_carry_crc[par] : 0xFFFFFFFFu;
        int len = marked ? 1 : 0;
        for (; i + len < n_el && !(w[len] & kSep) && (len == 0 || !((w[len] | w[len - 1]) & kAlone)); ++len)
          crc = crc_cp(s_crc, crc, w[len] & kCpMask);
        if (cut && i == last_start) {
          s_carry_crc[par ^ 1] = crc;
          s_cnt[i] = 0;
        } else {
          s_tok[i] = a.hash_lo + (int)((crc ^ 0xFFFFFFFFu) % (uint32_t)a.hash_span);
        }
        continue;
      }
      int len = 1;
      if (!(w[0] & kAlone))
        for (; len <= kMaxWord && i + len < n_el && !(w[len] & (kSep | kAlone)); ++len) {}
      if (marked || len > kMaxWord) { s_tok[i] = a.unk; continue; }
      int n_out = 0, start = 0;
      while (start < len) {
        uint32_t h = start ? kSeedCont : kSeedWord;
        int best = -1, best_end = start;
        const int lim = (len < start + a.lmax) ? len : start + a.lmax;
        for (int e = start; e < lim; ++e) {
          h = (h ^ (w[e] & kCpMask)) * kFnvPrime;
          const int id = vocab_find(a, w + start, e + 1 - start, start ? 1u : 0u, h);
          if (id >= 0) { best = id; best_end = e + 1; }
        }
        if (best_end == start) { n_out = -1; break; }
        s_tok[i + n_out++] = best;
        start = best_end;
      }
      if (n_out < 0) { s_tok[i] = a.unk; n_out = 1; }
      s_cnt[i] = (uint16_t)n_out;
    }
    __syncthreads();

    // 4. place the ids
    int mine = 0;
    const int lo = tid * kPerThread, hi = (lo + kPerThread < n_el) ? lo + kPerThread : n_el;
    for (int i = lo; i < hi; ++i) mine += s_cnt[i];
    int tile_tok;
    int at = n_tok + block_scan(mine, s_scan, &tile_tok);
    for (int i = lo; i < hi; ++i)
      for (int k = 0, c = s_cnt[i]; k < c; ++k, ++at)
        if (at < budget) out[1 + at] = s_tok[i + k];
    n_tok += tile_tok;

    // the cut word goes to the front
    carry = 0;
    if (cut) {
      const int len = n_el - last_start;
      const bool marked = (s_elems[last_start] & kMark) != 0;
      uint32_t keep = 0;
      const bool as_chars = a.mode == 0 && !marked && len <= kMaxWord;
      if (as_chars && tid < len) keep = s_elems[last_start + tid];
      __syncthreads();
      if (as_chars) {
        if (tid < len) s_elems[tid] = keep;
        carry = len;
      } else {
        if (tid == 0) s_elems[0] = kMark;
        carry = 1;
      }
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

int wordpiece_encode_launch(const uint8_t* text, const int64_t* offsets, int n_texts, int64_t n_bytes, const uint32_t* table,
                            int64_t table_len, const uint32_t* rep, int64_t rep_len, const int32_t* slots, int64_t n_slots,
                            const uint32_t* pool, int64_t pool_len, int max_probe, int lmax, int mode, int unk, int cls, int sep, int pad,
                            int hash_lo, int hash_span, int max_len, int* ids, int* lens, int* flags, hipStream_t stream) {
  Args a;
  a.text = text; a.offsets = offsets; a.n_bytes = n_bytes;
  a.table = table; a.table_len = table_len; a.rep = rep; a.rep_len = rep_len;
  a.slots = reinterpret_cast<const int4*>(slots); a.slot_mask = (uint32_t)(n_slots - 1);
  a.pool = pool; a.pool_len = pool_len;
  a.max_probe = max_probe; a.lmax = lmax; a.mode = mode; a.unk = unk; a.cls = cls; a.sep = sep; a.pad = pad;
  a.hash_lo = hash_lo; a.hash_span = hash_span; a.max_len = max_len;
  a.ids = ids; a.lens = lens; a.flags = flags;
  hipLaunchKernelGGL(wordpiece_kernel, dim3(n_texts), dim3(kThreads), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace crs
