// LZBuffer's codes on the MI355X -- the stream compressBlock's LZ77 pre-processor hands the coder, written from the list of
// matches lz77_walk_kernel leaves behind either parse (device/lz77_kernel.h, device/lz77_hash_kernel.h).  The specification is
// host/preproc.cpp Lz77::emit_tokens (LZBuffer's literals() / match(), libzpaq.cpp:6759-6883): byte for byte the same stream.
//
// A block's stream is a sequence of ITEMS, one per token and one for the end of the block.  With `prev` the end of the previous
// match (0 at the start) and `stop` the token's position (n for the end item), g = stop - prev literal steps precede it:
//   g / 4096 runs of exactly 4096 literals (the flush at kLzMaxLiteral), one run of g % 4096 + blit literals if that is not 0,
//   then the match (len, off) -- nothing for the end item.
// So an item's length follows from its token and its predecessor's end alone, its place from a prefix sum, and every literal
// byte's place from the item that covers it:
//
//   lzc_len_kernel       one lane per item slot (tok_cap + 1 per block): emit_tokens' checks, then the item's length in bits
//   (exclusive scan)     rocPRIM, 64-bit, in device/sa_kernels.hip
//   lzc_sizes_kernel     one lane per block: its stream's length in bytes
//   -- the host reads the sizes and the error word, places the streams and checks capacity --
//   lzc_match_kernel     one lane per token: the match's code
//   lzc_literal_kernel   one lane per input position: the token that covers it by binary search over the block's positions; a
//                        literal writes its 8 bits, the first literal of a run the run's header as well
//
// Level 2 is byte-aligned: every byte is stored by exactly one lane.  Level 1 is bit-packed, least significant bit first: the
// output is zeroed and only ever OR-ed (atomicOr on 32-bit words; integer OR does not depend on the order of arrival).
// No lane reads the input anywhere but at its own position, and the emitting kernels run only when no check failed.
#pragma once
#include "lz77_kernel.h"

namespace zpq {

static const uint32_t kLzcFullRunBits = 3u + 2u * 12u + 8u * kLzMaxLiteral;    // a run of 4096 literals at level 1
static_assert(kLzMaxLiteral == 4096u && kLzMaxLiteral % 64u == 0, "the flush must fall on a level-2 run boundary");

__device__ __forceinline__ uint64_t lzc_first_slot(const LzBlock* blocks, uint32_t b) { return blocks[b].tok_off + b; }

// the block whose slots hold slot s: the last one that starts at or below it (a block has at least one slot)
__device__ __forceinline__ uint32_t lzc_block_of_slot(const LzBlock* blocks, uint32_t nblocks, uint64_t s) {
  uint32_t lo = 0, hi = nblocks;
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (blocks[mid].tok_off + mid <= s) lo = mid; else hi = mid; }
  return lo;
}

// Item t of a block with cnt tokens (t <= cnt): emit_tokens' checks of token t and of the order behind token t - 1.  false: the
// host refuses this list.  prev = end of the previous match, stop = where the literal steps end, k = the token (zeros for the
// end item).  No field is used before it is checked; the sums are 64-bit.
__device__ __forceinline__ bool lzc_item(const LzBlock& B, const LzTok* tk, uint32_t cnt, uint32_t t, uint32_t& prev, uint32_t& stop, LzTok& k) {
  uint64_t p = 0;
  if (t) { const LzTok q = tk[t - 1]; p = (uint64_t)q.i + q.blit + q.len; }
  k.i = k.off = k.len = k.blit = 0;
  if (p > B.n) return false;
  prev = (uint32_t)p;
  stop = B.n;
  if (t == cnt) return true;
  k = tk[t];
  if (k.i < prev || k.i > B.n) return false;
  if (k.off == 0 || k.off > k.i || k.len == 0 || (uint64_t)k.i + k.blit + k.len > B.n) return false;
  stop = k.i;
  return true;
}

__device__ __forceinline__ uint32_t lzc_lit_header_bits(uint32_t lit) { return 3u + 2u * (uint32_t)(lz_bit_length(lit) - 1); }

// bits of the literal runs of an item: g steps in front, blit more that belong to the match
__device__ __forceinline__ uint64_t lzc_literal_bits(uint32_t level, uint32_t g, uint32_t blit) {
  const uint64_t nfull = g / kLzMaxLiteral;
  const uint64_t lit = (uint64_t)(g % kLzMaxLiteral) + blit;
  if (level == 1) return nfull * kLzcFullRunBits + (lit ? lzc_lit_header_bits((uint32_t)lit) + 8u * lit : 0u);
  return 8u * (nfull * (kLzMaxLiteral + kLzMaxLiteral / 64u) + lit + (lit + 63u) / 64u);
}

// level 1: the offset as match() codes it -- off' = off + 2^rb - 1, lo = bits of off' >> rb below its leading one
__device__ __forceinline__ uint32_t lzc_offset_lo(uint32_t off, uint32_t rb, uint32_t& offp) {
  offp = off + (1u << rb) - 1u;
  return (uint32_t)lz_bit_length(offp) - 1u - rb;
}

// level 2: the pieces match() splits a length into (at most min_match + 63 each, the last two share what is left)
__device__ __forceinline__ uint32_t lzc_piece(uint32_t len, uint32_t mm) {
  return len > mm * 2u + 63u ? mm + 63u : (len > mm + 63u ? len - mm : len);
}
__device__ __forceinline__ uint64_t lzc_pieces(uint32_t len, uint32_t mm) {
  const uint32_t P = mm + 63u, two = mm * 2u + 63u;
  uint64_t np = 0;
  if (len > two) { np = ((uint64_t)(len - two) + P - 1u) / P; len -= (uint32_t)np * P; }     // (what is left lies in (mm, two])
  return np + (len > P ? 2u : 1u);
}
__device__ __forceinline__ uint32_t lzc_piece_bytes(uint32_t off) { return off - 1u < (1u << 16) ? 3u : (off - 1u < (1u << 24) ? 4u : 5u); }

__device__ __forceinline__ uint64_t lzc_match_bits(const LzBlock& B, const LzTok& k) {
  if (B.kind == 1) {
    uint32_t offp;
    const uint32_t lo = lzc_offset_lo(k.off, B.rb, offp);
    const int lb = lz_bit_length(k.len);
    return 8u + 2u * (uint32_t)(lb > 3 ? lb - 3 : 0) + B.rb + lo;
  }
  return 8u * lzc_pieces(k.len, B.min_match) * lzc_piece_bytes(k.off);
}

// (a) one lane per item slot, and one more for the sum behind the last
__device__ __forceinline__ void lzc_len_body(const LzBlock* blocks, uint32_t nblocks, uint64_t nslots, const LzTok* toks, const uint32_t* counts,
                                             uint64_t* len, uint32_t* err) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s > nslots) return;
  uint64_t bits = 0;
  if (s < nslots) {
    const uint32_t b = lzc_block_of_slot(blocks, nblocks, s);
    const LzBlock B = blocks[b];
    const uint32_t t = (uint32_t)(s - (B.tok_off + b)), cnt = counts[b];
    if (B.kind == 1 || B.kind == 2) {
      if (cnt > B.tok_cap) {                                      // (the list is incomplete: lz77_walk_body)
        if (t == 0) atomicOr(err, kLzcErrCount);
      } else if (t <= cnt) {
        uint32_t prev, stop;
        LzTok k;
        if (!lzc_item(B, toks + B.tok_off, cnt, t, prev, stop, k)) atomicOr(err, kLzcErrList);
        else bits = lzc_literal_bits(B.kind, stop - prev, k.blit) + (t < cnt ? lzc_match_bits(B, k) : 0u);
      }
    }
  }
  len[s] = bits;
}

// (b') one lane per block: bytes of its stream (the last partial byte of level 1 is padded with zero bits)
__device__ __forceinline__ void lzc_sizes_body(const LzBlock* blocks, uint32_t nblocks, uint64_t nslots, const uint64_t* pos, uint32_t* sizes) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nblocks) return;
  const uint64_t from = pos[lzc_first_slot(blocks, b)], to = pos[b + 1u < nblocks ? lzc_first_slot(blocks, b + 1u) : nslots];
  const uint64_t bytes = (to - from + 7u) >> 3;
  sizes[b] = bytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)bytes;
}

// nb <= 57 bits of v at bit `at` of a zeroed, word-aligned stream; nothing at or behind bit `end` is touched
__device__ __forceinline__ void lzc_or_bits(uint32_t* out, uint64_t at, uint64_t end, uint64_t v, uint32_t nb) {
  if (at + nb > end) return;
  const uint64_t w = at >> 5;
  const uint32_t sh = (uint32_t)at & 31u;
  const uint32_t a = (uint32_t)(v << sh);
  if (a) atomicOr(out + w, a);
  if (sh + nb > 32u) {
    const uint64_t rest = v >> (32u - sh);
    if ((uint32_t)rest) atomicOr(out + w + 1u, (uint32_t)rest);
    if ((uint32_t)(rest >> 32)) atomicOr(out + w + 2u, (uint32_t)(rest >> 32));
  }
}

// the header of a run of lit literals at level 1: 00, the length as interleaved Elias gamma (leading one implied), 0
__device__ __forceinline__ uint64_t lzc_lit_header(uint32_t lit) {
  uint64_t v = 0;
  uint32_t nb = 2;
  for (int ll = lz_bit_length(lit) - 2; ll >= 0; --ll) {
    v |= 1ull << nb;
    v |= (uint64_t)((lit >> ll) & 1u) << (nb + 1u);
    nb += 2u;
  }
  return v;
}

// Where block b's stream lies: out_off[b] bytes into `out` (a multiple of 4), out_off[b + 1] its end (of the block's room, not of
// its stream: the bound no store crosses).
// (d.1) one lane per token slot: the match's code behind the item's literals
__device__ __forceinline__ void lzc_match_body(const LzBlock* blocks, uint32_t nblocks, uint64_t nslots, const LzTok* toks, const uint32_t* counts,
                                               const uint64_t* pos, const uint64_t* out_off, uint8_t* out) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nslots) return;
  const uint32_t b = lzc_block_of_slot(blocks, nblocks, s);
  const LzBlock B = blocks[b];
  const uint64_t first = B.tok_off + b;
  const uint32_t t = (uint32_t)(s - first), cnt = counts[b];
  if ((B.kind != 1 && B.kind != 2) || cnt > B.tok_cap || t >= cnt) return;
  uint32_t prev, stop;
  LzTok k;
  if (!lzc_item(B, toks + B.tok_off, cnt, t, prev, stop, k)) return;
  const uint64_t base = out_off[b] * 8u, end = out_off[b + 1u] * 8u;
  uint64_t at = base + (pos[s] - pos[first]) + lzc_literal_bits(B.kind, stop - prev, k.blit);
  if (B.kind == 1) {                  // mm,mmm,n,ll,r,q: length 4n+ll at offset ((q-1) << rb) + r + 1
    uint32_t offp;
    const uint32_t lo = lzc_offset_lo(k.off, B.rb, offp);
    uint64_t v = ((lo + 8u) >> 3) & 3u;
    v |= (uint64_t)(lo & 7u) << 2;
    uint32_t nb = 5;
    for (int ll = lz_bit_length(k.len) - 2; ll >= 2; --ll) {
      v |= 1ull << nb;
      v |= (uint64_t)((k.len >> ll) & 1u) << (nb + 1u);
      nb += 2u;
    }
    ++nb;
    v |= (uint64_t)(k.len & 3u) << nb;
    nb += 2u;
    lzc_or_bits((uint32_t*)out, at, end, v, nb);
    const uint32_t ob = B.rb + lo;                                // r and q lie side by side: the bits of off' below its leading one
    lzc_or_bits((uint32_t*)out, at + nb, end, (uint64_t)offp & ((1ull << ob) - 1u), ob);
  } else {                            // yyxxxxxx + y+1 offset bytes, length x + minimum match; long matches are split
    const uint32_t off = k.off - 1u, pb = lzc_piece_bytes(k.off);
    uint64_t p = at >> 3;
    uint32_t len = k.len;
    while (len > 0 && p + pb <= (end >> 3)) {
      const uint32_t len1 = lzc_piece(len, B.min_match);
      out[p++] = (uint8_t)(64u * (pb - 2u) + len1 - B.min_match);
      if (pb > 4u) out[p++] = (uint8_t)(off >> 24);
      if (pb > 3u) out[p++] = (uint8_t)(off >> 16);
      out[p++] = (uint8_t)(off >> 8);
      out[p++] = (uint8_t)off;
      len -= len1;
    }
  }
}

// (d.2) one lane per input position
__device__ __forceinline__ void lzc_literal_body(const uint8_t* in_all, const LzBlock* blocks, uint32_t nblocks, uint64_t total, const LzTok* toks,
                                                 const uint32_t* counts, const uint64_t* pos, const uint64_t* out_off, uint8_t* out) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  uint32_t b = 0, hb = nblocks;                    // the last block that starts at or below e (empty blocks share their start with the next)
  while (hb - b > 1) { const uint32_t mid = (b + hb) >> 1; if (blocks[mid].off <= e) b = mid; else hb = mid; }
  const LzBlock B = blocks[b];
  const uint32_t j = (uint32_t)(e - B.off), cnt = counts[b];
  if ((B.kind != 1 && B.kind != 2) || j >= B.n || cnt > B.tok_cap) return;
  const LzTok* tk = toks + B.tok_off;
  uint32_t lo = 0, hi = cnt;                       // tokens that stand at or below j (their positions rise strictly)
  while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (tk[mid].i <= j) lo = mid + 1u; else hi = mid; }
  uint32_t u = 0;                                  // the item whose literal runs hold j
  if (lo) {
    const LzTok q = tk[lo - 1u];
    if (j - q.i < q.blit) u = lo - 1u;                            // a literal in front of the match that belongs to it
    else if (j - q.i - q.blit < q.len) return;                    // inside the match
    else u = lo;
  }
  uint32_t prev, stop;
  LzTok k;
  if (!lzc_item(B, tk, cnt, u, prev, stop, k)) return;
  const uint64_t first = B.tok_off + b;
  const uint64_t base = out_off[b] * 8u + (pos[first + u] - pos[first]), end = out_off[b + 1u] * 8u;
  const uint32_t g = stop - prev, d = j - prev;
  const uint32_t byte = in_all[e];
  if (B.kind == 1) {
    const uint32_t nfull = g / kLzMaxLiteral;
    uint64_t at;
    uint32_t lit, r;
    if (d / kLzMaxLiteral < nfull) { at = base + (uint64_t)(d / kLzMaxLiteral) * kLzcFullRunBits; lit = kLzMaxLiteral; r = d % kLzMaxLiteral; }
    else { at = base + (uint64_t)nfull * kLzcFullRunBits; lit = g % kLzMaxLiteral + k.blit; r = d - nfull * kLzMaxLiteral; }
    const uint32_t hbits = lzc_lit_header_bits(lit);
    if (r == 0) lzc_or_bits((uint32_t*)out, at, end, lzc_lit_header(lit), hbits);
    lzc_or_bits((uint32_t*)out, at + hbits + 8ull * r, end, byte, 8u);
  } else {
    // runs of 64: the flush falls on a run boundary, so the item's g + blit literals are cut as one sequence
    const uint32_t L = g + k.blit, r = d & 63u;
    const uint64_t p = (base >> 3) + (uint64_t)(d >> 6) * 65u;
    if (p + 2u + r > (end >> 3)) return;
    if (r == 0) out[p] = (uint8_t)((L - d < 64u ? L - d : 64u) - 1u);
    out[p + 1u + r] = (uint8_t)byte;
  }
}

}  // namespace zpq
