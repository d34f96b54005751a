// The LZ77 parse through LZBuffer's hash table on the MI355X -- compressBlock's pre-processor of method 1, of method 2 for
// blocks of type below 64 and of every x / s method with args[5] - args[0] < 21 (LZBuffer::fill without a suffix array,
// libzpaq.cpp:6702-6782; host/preproc.cpp Lz77::run states it).
//
// The reference keeps one table of 2^args[5] slots, looks a position up in it and then indexes the bytes it steps over.  Three
// properties of that code make the search a function of the position:
//   1. every byte stepped over is indexed, after a literal as after a match: when position i is searched, slot s holds the
//      latest j < min(i, U) whose insertion slot is s (U = max(0, n - minMatchBoth): nothing is indexed from there on);
//   2. the rolling hashes forget: a byte has left the table mask after minMatch (minMatch2) updates, so the hash in front of
//      position t is the recurrence run from 0 over the last min(t, minMatch) updates; they stand still from U on;
//   3. of the parse so far only one bit enters a search: whether literals are pending.
// So the table becomes a sorted array of keys  block << 48 | slot << 24 | j  and "what does slot s hold at position i" the
// predecessor of (block, s, i) in it:
//
//   lzh_keys_kernel     one lane per position j < U of every block: its one or two insertion slots as keys (and the block
//                       of every element, for the search)
//   (radix sort)        rocPRIM, in device/sa_kernels.hip
//   lzh_index_kernel    one lane per sorted key: where the keys of every slot prefix of a block start -- the slots one search
//                       reads (h ^ k, k = 0 .. bucket) share their prefix, so a search reads two index entries and then looks
//                       for predecessors among the few keys between them, not in the whole array
//   lzh_search_kernel   one lane per position: the reference's two loops statement for statement, for both values of the
//                       pending-literals bit over the same candidates; the decision word of lz77_search_body
//   lz77_walk_kernel    (device/lz77_kernel.h, unchanged) follows the chain and lists the matches taken
//
// Bit-exact by construction; the emulator runs this file against the host's parse (tests/emu/lz77_hash_emu_main.cpp), the GPU
// tests against the reference's archives.
#pragma once
#include "lz77_kernel.h"

namespace zpq {

static const uint32_t kLzhMaxTableBits = 24u;        // a slot number fits the key's 24 bits
static const uint32_t kLzhNone = 0xFFFFFFFFu;

// h1 / h2 as LZBuffer::fill holds them when it stands at position t <= ins_end
__device__ __forceinline__ uint32_t lzh_hash1(const uint8_t* in, uint32_t t, const LzBlock& B) {
  const uint32_t shift = (B.ht_bits - 1u) / B.min_match + 1u, m = t < B.min_match ? t : B.min_match;
  uint32_t h = 0;
  for (uint32_t j = t - m; j < t; ++j) h = ((h * 5u) << shift) + ((uint32_t)in[j + B.min_match] + 1u) * 123456791u;
  return h & ((1u << B.ht_bits) - 1u);
}
__device__ __forceinline__ uint32_t lzh_hash2(const uint8_t* in, uint32_t t, const LzBlock& B) {
  const uint32_t shift = (B.ht_bits - 1u) / B.min_match2 + 1u, m = t < B.min_match2 ? t : B.min_match2;
  uint32_t h = 0;
  for (uint32_t j = t - m; j < t; ++j) h = ((h * 9u) << shift) + ((uint32_t)in[j + B.min_match2 + B.lookahead] + 1u) * 23456789u;
  return h & ((1u << B.ht_bits) - 1u);
}

__device__ __forceinline__ bool lzh_block(const LzBlock& B) { return (B.kind == 1 || B.kind == 2) && B.ht_bits != 0; }

// One lane per element of the batch: its block, and for an inserted position its keys (two when there is a longer context: both
// hashes index the same table), at key_off + j x (1 or 2) -- in the order the reference writes them.
__device__ __forceinline__ void lzh_keys_body(const uint8_t* in_all, const LzBlock* blocks, uint32_t nblocks, uint64_t total, uint16_t* blk,
                                              uint64_t* keys) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  uint32_t lo = 0, hi = nblocks;                   // the last block that starts at or below e (empty blocks share their start with the next)
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (blocks[mid].off <= e) lo = mid; else hi = mid; }
  blk[e] = (uint16_t)lo;
  const LzBlock B = blocks[lo];
  const uint32_t j = (uint32_t)(e - B.off);
  if (!lzh_block(B) || j >= B.ins_end) return;
  const uint8_t* in = in_all + B.off;
  const uint32_t ih = ((j * 1234547u) >> 19) & B.bucket;
  const uint64_t top = (uint64_t)lo << 48;
  if (B.min_match2) {
    keys[B.key_off + 2ull * j] = top | (uint64_t)(lzh_hash2(in, j, B) ^ ih) << 24 | j;
    keys[B.key_off + 2ull * j + 1] = top | (uint64_t)(lzh_hash1(in, j, B) ^ ih) << 24 | j;
  } else {
    keys[B.key_off + j] = top | (uint64_t)(lzh_hash1(in, j, B) ^ ih) << 24 | j;
  }
}

// One lane per sorted key: idx[idx_off + c] = first key of the block (counted from key_off) whose slot prefix is c or more,
// for c = 0 .. 2^idx_bits.  A lane fills the entries between its left neighbour's prefix and its own; the block's last key the
// rest.  Blocks without keys have no lane: their index is never read.
__device__ __forceinline__ void lzh_index_body(const uint64_t* keys, uint64_t nkeys, const LzBlock* blocks, uint32_t* idx) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nkeys) return;
  const uint64_t key = keys[k];
  const LzBlock B = blocks[(uint32_t)(key >> 48)];
  const uint32_t sh = B.ht_bits - B.idx_bits, last = 1u << B.idx_bits;
  uint32_t c = ((uint32_t)(key >> 24) & 0xFFFFFFu) >> sh;
  if (c >= last) c = last - 1u;                    // (no slot is that large)
  const uint32_t rel = (uint32_t)(k - B.key_off);
  uint32_t* out = idx + B.idx_off;
  uint32_t from = 0;
  if (rel) {
    const uint32_t cp = ((uint32_t)(keys[k - 1] >> 24) & 0xFFFFFFu) >> sh;
    from = (cp < c ? cp : c) + 1u;
  }
  for (uint32_t cc = from; cc <= c; ++cc) out[cc] = rel;
  if (rel + 1u == B.nkeys)
    for (uint32_t cc = c + 1u; cc <= last; ++cc) out[cc] = B.nkeys;
}

// What the table's slot holds when the reference stands at position i: the latest inserted j < i, among keys[lo .. hi) of the
// block (the range of the slot's prefix).  kLzhNone: nothing was ever written there.
__device__ __forceinline__ uint32_t lzh_slot(const uint64_t* keys, uint32_t lo, uint32_t hi, uint64_t block_slot, uint32_t i) {
  const uint64_t target = block_slot << 24 | i;
  uint32_t a = lo, b = hi;                         // first key >= target
  while (a < b) { const uint32_t mid = a + ((b - a) >> 1); if (keys[mid] < target) a = mid + 1u; else b = mid; }
  if (a == lo) return kLzhNone;
  const uint64_t key = keys[a - 1u];
  return (key >> 24) == block_slot ? (uint32_t)key & 0xFFFFFFu : kLzhNone;
}

// The search LZBuffer::fill makes at position i of block b, for "literals pending" (r0) and "no literals pending" (r1): the
// decision words of lz_search.  `in`, `keys`, `idx` are the block's own.
__device__ __forceinline__ void lzh_search(const uint8_t* in, const uint64_t* keys, const uint32_t* idx, uint32_t b, uint32_t i, const LzBlock& B,
                                           uint2& r0, uint2& r1) {
  const uint32_t n = B.n, cb = B.checkbits, mask = (1u << cb) - 1u, la = B.lookahead, mm2 = B.min_match2;
  const uint32_t lim = n - i < kLzMaxMatch ? n - i : kLzMaxMatch;
  const uint32_t c3 = i + 3u < n ? in[i + 3u] : 0u;                // (the host's reads past the end see zeros; here the next block lies there)
  const uint32_t t = i < B.ins_end ? i : B.ins_end;
  const uint32_t sh = B.ht_bits - B.idx_bits;
  uint32_t blen[2], bp[2], blit[2];
  int bscore[2];
  for (int v = 0; v < 2; ++v) { blen[v] = B.min_match - 1u; bp[v] = 0; blit[v] = 0; bscore[v] = 0; }
  if (B.nkeys) {
    if (mm2) {                                                      // the longer context first
      const uint32_t h2 = lzh_hash2(in, t, B);
      const uint32_t lo = idx[h2 >> sh], hi = idx[(h2 >> sh) + 1u];
      bool on[2] = {true, true};
      for (uint32_t k = 0; k <= B.bucket && (on[0] || on[1]); ++k) {
        const uint32_t j = lo < hi ? lzh_slot(keys, lo, hi, (uint64_t)b << 24 | (h2 ^ k), i) : kLzhNone;
        if (j != kLzhNone) {
          const uint32_t p32 = (j << cb) | ((uint32_t)in[j + 3u] & mask);        // the table entry, 32 bits as the reference keeps it
          if (p32 && (p32 & mask) == (c3 & mask)) {
            const uint32_t p = p32 >> cb;
            bool ok[2];
            for (int v = 0; v < 2; ++v) ok[v] = on[v] && p < i && i + blen[v] <= n && in[p + blen[v] - 1u] == in[i + blen[v] - 1u];
            if (ok[0] || ok[1]) {
              const uint32_t l = la < lim ? lz_match_end(in, p, i, la, lim) : la;
              if (l >= mm2 + la) {
                uint32_t l1 = la;
                while (l1 > 0 && in[p + l1 - 1u] == in[i + l1 - 1u]) --l1;
                const int base = (int)(l - l1) * 8 - lz_bit_length(i - p) - 11;
                for (int v = 0; v < 2; ++v) {
                  if (!ok[v]) continue;
                  const int score = base - ((v == 1 && l1 > 0) ? 8 : 0);
                  if (score > bscore[v]) { blen[v] = l; bp[v] = p; blit[v] = l1; bscore[v] = score; }
                }
              }
            }
          }
        }
        for (int v = 0; v < 2; ++v) if (blen[v] >= 128u) on[v] = false;
      }
    }
    bool on[2];
    for (int v = 0; v < 2; ++v) on[v] = !mm2 || blen[v] < mm2;
    if (on[0] || on[1]) {
      const uint32_t h1 = lzh_hash1(in, t, B);
      const uint32_t lo = idx[h1 >> sh], hi = idx[(h1 >> sh) + 1u];
      for (uint32_t k = 0; k <= B.bucket && (on[0] || on[1]); ++k) {
        const uint32_t j = (lo < hi && i + 3u < n) ? lzh_slot(keys, lo, hi, (uint64_t)b << 24 | (h1 ^ k), i) : kLzhNone;
        if (j != kLzhNone) {
          const uint32_t p32 = (j << cb) | ((uint32_t)in[j + 3u] & mask);
          if (p32 && (p32 & mask) == (c3 & mask)) {
            const uint32_t p = p32 >> cb;
            bool ok[2];
            for (int v = 0; v < 2; ++v) ok[v] = on[v] && p < i && i + blen[v] <= n && in[p + blen[v] - 1u] == in[i + blen[v] - 1u];
            if (ok[0] || ok[1]) {
              const uint32_t l = lz_match_end(in, p, i, 0, lim);
              const int base = (int)l * 8 - lz_bit_length(i - p) - 11;
              for (int v = 0; v < 2; ++v) {
                if (!ok[v]) continue;
                const int score = base - (v == 0 ? 2 : 0);
                if (score > bscore[v]) { blen[v] = l; bp[v] = p; blit[v] = 0; bscore[v] = score; }
              }
            }
          }
        }
        for (int v = 0; v < 2; ++v) if (blen[v] >= 128u) on[v] = false;
      }
    }
  }
  uint2 r[2];
  for (int v = 0; v < 2; ++v) {
    const uint32_t off = i - bp[v];
    const uint32_t need = B.min_match + (B.kind == 2 ? (uint32_t)(off >= (1u << 16)) + (uint32_t)(off >= (1u << 24)) : 0u);
    const bool take = off > 0 && bscore[v] > 0 && blen[v] - blit[v] >= need;
    r[v].x = take ? off : 0u;
    r[v].y = take ? ((blen[v] - blit[v]) | (blit[v] & kLzMaxLookahead) << 16 | 1u << 31) : 0u;
  }
  r0 = r[0];
  r1 = r[1];
}

__device__ __forceinline__ void lzh_search_body(const uint8_t* in_all, const uint64_t* keys, const uint32_t* idx, const uint16_t* blk,
                                                const LzBlock* blocks, uint64_t total, uint4* res) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const uint32_t b = blk[e];
  const LzBlock B = blocks[b];
  if (!lzh_block(B)) return;
  uint2 r0, r1;
  lzh_search(in_all + B.off, keys + B.key_off, idx + B.idx_off, b, (uint32_t)(e - B.off), B, r0, r1);
  uint4 r;
  r.x = r0.x; r.y = r0.y; r.z = r1.x; r.w = r1.y;
  res[e] = r;
}

}  // namespace zpq
