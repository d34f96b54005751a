// The LZ77 parse of ONE block of any length below 2^31 behind the wide suffix sort (device/sa_wide_kernel.h) -- what
// lz77_search_kernel and lz77_walk_kernel (device/lz77_kernel.h) do for a batch of blocks below 2^24, for a block that fills the
// device alone.  The search is the same per position (lz_search); there is no element-to-block map.  The walk is one wavefront
// per block there, which for one block is one wavefront on the whole machine.  It is serial only in appearance:
//
//   the walk's whole state is (i, lit): the position and the literals pending (0 .. kLzMaxLiteral - 1).  Behind every match it
//   takes the state is (i, 0).  Two walks that reach the same state are the same walk from there on.
//
// So the block is cut into pieces of P positions:
//
//   lz77_wide_search   one lane per position: the 16-byte decision word (lz_search, both values of "literals pending")
//   lz77_wide_walk     one wavefront per piece: piece k is walked from the PROVISIONAL state (k P, 0) with lz77_walk_body's
//                      transition until i >= min((k + 1) P, n); its tokens go to its own slots, then {count, exit state}
//   lz77_wide_stitch   one wavefront runs the pieces in order with the TRUE state and the running count.  The state is past the
//                      piece: nothing.  The state is (k P, 0): the piece's list is the truth, the state becomes its exit state.
//                      Otherwise it walks on from the true state, writing into the final list, and behind every match it takes
//                      it looks (binary search: the ends rise strictly) whether its position is the end of one of the piece's
//                      tokens: from there on the piece's list is the truth.  No such position before the piece's end: only its
//                      own tokens count.  A list is adopted only at an identical state, so the final list is the single walk's
//                      by construction; re-joining is never needed for that -- data that never re-joins is walked serially.
//   lz77_wide_gather   one workgroup per piece: its adopted tokens are copied to their place in the final list
//
// No kernel waits for another workgroup; the cross-lane traffic is v_readlane and the ballot (tests/emu/wave_emu.h models both:
// tests/emu/lz77_wide_emu_main.cpp runs these bodies against the host's parse).
#pragma once
#include "lz77_kernel.h"
#include "lz77_wide_layout.h"

namespace zpq {

__device__ __forceinline__ void lz77_wide_search_body(const uint8_t* in, const uint32_t* sa, const uint32_t* rank, const LzBlock* blocks, uint4* res) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const LzBlock B = blocks[0];
  if (e >= B.n || (B.kind != 1 && B.kind != 2)) return;
  uint2 r0, r1;
  lz_search(in, B.n, sa, rank, (uint32_t)e, B, r0, r1);
  uint4 r;
  r.x = r0.x; r.y = r0.y; r.z = r1.x; r.w = r1.y;
  res[e] = r;
}

__device__ __forceinline__ uint32_t lz_wide_tok_end(const LzTok& t) { return t.i + t.blit + t.len; }

// lz77_walk_body's loop from the state (i, lit) until i >= stop (stop <= n): 64 decisions per load, the pending-takes ballot, a
// run of literals as one step, the flush.  Tokens go to toks[nt] while nt < cap; nt counts on.  Every lane of the wavefront is
// here and holds the same state.  REJOIN: behind every match taken, a position below `stop` that is the end of one of the pc
// tokens at prov ends the walk -- true, joined = that token.
template <bool REJOIN>
__device__ __forceinline__ bool lz_wide_walk(const uint4* r, uint32_t n, uint32_t stop, uint32_t& i, uint32_t& lit, LzTok* toks, uint32_t& nt, uint32_t cap,
                                             int lane, const LzTok* prov, uint32_t pc, uint32_t& joined) {
  while (i < stop) {
    const uint32_t base = i;
    uint4 e;
    e.x = e.y = e.z = e.w = 0;
    if (base + (uint32_t)lane < n) e = r[base + (uint32_t)lane];
    // positions of this chunk where a match is taken although literals are pending
    const unsigned long long pending_takes = __builtin_amdgcn_ballot_w64((e.y >> 31) != 0u);
    while (i < stop && i - base < 64u) {
      const int src = (int)(i - base);
      if (lit != 0) {
        // a run of literals in one step: up to the next such position, the end of the chunk or of the piece, or the flush
        const unsigned long long ahead = pending_takes >> src;
        uint32_t d = ahead ? (uint32_t)__builtin_ctzll(ahead) : 64u - (uint32_t)src;
        d = d < stop - i ? d : stop - i;
        d = d < kLzMaxLiteral - lit ? d : kLzMaxLiteral - lit;
        if (d) {
          i += d;
          lit += d;
          if (lit >= kLzMaxLiteral) lit = 0;
          continue;
        }
      }
      const bool none = lit == 0;                                    // (the same in every lane)
      const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)(none ? e.z : e.x), src);
      const uint32_t y = (uint32_t)__builtin_amdgcn_readlane((int)(none ? e.w : e.y), src);
      if (y >> 31) {
        const uint32_t len = y & 0xFFFFu, front = (y >> 16) & 0xFFu;
        if (lane == 0 && nt < cap) {
          LzTok t;
          t.i = i; t.off = x; t.len = len; t.blit = front;
          toks[nt] = t;
        }
        ++nt;
        lit = 0;
        i += front + len;
        if (REJOIN && i < stop) {
          uint32_t lo = 0, hi = pc;                                  // the first provisional token that ends at or behind i
          while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (lz_wide_tok_end(prov[mid]) < i) lo = mid + 1u; else hi = mid;
          }
          if (lo < pc && lz_wide_tok_end(prov[lo]) == i) { joined = lo; return true; }
        }
      } else {
        ++lit;
        ++i;
        if (lit >= kLzMaxLiteral) lit = 0;                           // (flushed: LZBuffer::fill)
      }
    }
  }
  return false;
}

__device__ __forceinline__ uint32_t lz_wide_piece_stop(const LzWideParams& W, uint32_t k) {
  const uint64_t end = ((uint64_t)k + 1u) * W.piece;
  return end < W.n ? (uint32_t)end : W.n;
}

// One wavefront per piece (64 threads per workgroup)
__device__ __forceinline__ void lz77_wide_walk_body(LzWideParams W, const uint4* res, LzTok* prov, LzWidePiece* pieces) {
  const uint32_t k = blockIdx.x;
  if (k >= W.npieces) return;
  const int lane = (int)(threadIdx.x & 63u);
  uint32_t i = k * W.piece, lit = 0, nt = 0, joined = 0;
  (void)lz_wide_walk<false>(res, W.n, lz_wide_piece_stop(W, k), i, lit, prov + (uint64_t)k * W.slot_cap, nt, W.slot_cap, lane, nullptr, 0u, joined);
  if (lane == 0) {
    LzWidePiece p;
    p.count = nt; p.exit_i = i; p.exit_lit = lit; p.pad = 0;
    pieces[k] = p;
  }
}

// One wavefront for the block.  toks: the final list, tok_cap slots.
__device__ __forceinline__ void lz77_wide_stitch_body(LzWideParams W, const uint4* res, const LzTok* prov, const LzWidePiece* pieces, LzTok* toks,
                                                      uint32_t tok_cap, LzWideAdopt* adopt, LzWideResult* out) {
  const int lane = (int)(threadIdx.x & 63u);
  uint32_t i = 0, lit = 0, nt = 0, whole = 0, rejoined = 0, own = 0, overflow = 0;
  for (uint32_t k = 0; k < W.npieces; ++k) {
    const uint32_t stop = lz_wide_piece_stop(W, k);
    LzWideAdopt a;
    a.first = 0; a.count = 0; a.how = kLzWideOwn;
    if (i < stop) {
      const LzWidePiece p = pieces[k];
      const bool ok = p.count <= W.slot_cap;
      if (!ok) overflow = 1;
      if (ok && lit == 0 && i == k * W.piece) {
        a.count = p.count; a.how = kLzWideWhole;
        i = p.exit_i; lit = p.exit_lit;
      } else {
        uint32_t joined = 0;
        if (lz_wide_walk<true>(res, W.n, stop, i, lit, toks, nt, tok_cap, lane, prov + (uint64_t)k * W.slot_cap, ok ? p.count : 0u, joined)) {
          a.first = joined + 1u; a.count = p.count - (joined + 1u); a.how = kLzWideRejoined;
          i = p.exit_i; lit = p.exit_lit;
        }
      }
    }
    a.dst = nt;
    nt += a.count;
    whole += a.how == kLzWideWhole;
    rejoined += a.how == kLzWideRejoined;
    own += a.how == kLzWideOwn;
    if (lane == 0) adopt[k] = a;
  }
  if (lane == 0) {
    LzWideResult r;
    r.count = nt; r.pieces = W.npieces; r.how[0] = whole; r.how[1] = rejoined; r.how[2] = own; r.overflow = overflow; r.pad[0] = r.pad[1] = 0;
    *out = r;
  }
}

// One workgroup per piece: its lanes copy the piece's adopted tokens, a stride of the workgroup apart
__device__ __forceinline__ void lz77_wide_gather_body(LzWideParams W, const LzTok* prov, const LzWideAdopt* adopt, LzTok* toks, uint32_t tok_cap) {
  const uint32_t k = blockIdx.x;
  if (k >= W.npieces) return;
  const LzWideAdopt a = adopt[k];
  if ((uint64_t)a.first + a.count > W.slot_cap) return;
  const LzTok* from = prov + (uint64_t)k * W.slot_cap + a.first;
  for (uint32_t t = threadIdx.x; t < a.count; t += blockDim.x)
    if ((uint64_t)a.dst + t < tok_cap) toks[a.dst + t] = from[t];
}

}  // namespace zpq
