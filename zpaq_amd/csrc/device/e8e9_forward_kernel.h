// The forward E8E9 filter on the MI355X -- what e8e9_forward of host/preproc.cpp (libzpaq.cpp:6450-6459) computes, for a batch of
// blocks that lie in one device buffer, in place.  The scan walks i from n - 5 down to 0, tests (b[i] & 254) == 0xe8 and
// ((b[i + 4] + 1) & 254) == 0, and a hit rewrites b[i + 1 .. i + 3] (the address plus i, mod 2^24).  It is serial only along short
// chains, in the mirror image of device/e8e9_kernel.h:
//
//   - a hit at j writes j + 1 .. j + 3 and only j > i ran when i is visited, so b[i] is still original there:
//     cand(i) = i + 4 < n && orig[i] in {e8, e9} is known for every position at once.  The tail byte b[i + 4] is the one that may
//     have been rewritten (in the inverse it is the opcode byte);
//   - only a hit at i + 1 .. i + 3 can change what i sees.  A BREAK is a candidate with no candidate in the three positions
//     behind it; a CHAIN runs downward from a break to the last candidate above the next lower break.  Chains neither read nor
//     write each other's bytes, given that a walk stops four positions above the next lower break (the three below that are no
//     candidates, and the lower chain's first hit rewrites them);
//   - a SEED is a candidate whose original b[i + 4] is 00 / ff.  More than three positions below its last hit a walk sees
//     original bytes only, so the next possible hit is the next lower seed, and a chain without a seed has no hit.
//
//   e8f_mark_kernel       a lane per 16 bytes (20 bytes loaded), a workgroup of 256 per tile of kE8Tile bytes: the seed and break
//                         flags of the lane's positions, their counts summed over the tile -> cnt[tile], cnt[ntiles + tile];
//                         status[block] = 0.
//   -- an exclusive scan over the 2 * ntiles + 1 counts (rocPRIM); the host reads the two totals and sizes the list --
//   e8f_scatter_kernel    the same flags again (the bytes are still original) and a prefix over the workgroup's lanes: the
//                         positions of the seeds, then of the breaks, into one list, sorted per block.
//   e8f_walk_kernel       a lane per seed.  A seed is a HEAD when a break lies in [seed, next higher seed): one binary search; the
//                         others leave.  A head tests and rewrites position by position, downward, while a hit is at most 3
//                         above, else jumps to the next lower seed, and ends when that lies at or below the next lower break.
//                         The rewritten bytes go out as byte stores: neighbouring chains may share a word.  After max_steps
//                         steps a lane gives up and sets status[block] = 1: the block is declined and nothing of it may be used.
//
// PLACEMENT.  The blocks lie where the sorters and the parsers want them: back to back, E8Block::off any byte offset, no room
// rounded up.  The mark pass tolerates that: a lane with 20 bytes of its block in front of it loads them as 16 + 4 at whatever
// alignment (global loads need none on gfx950), a lane nearer the block's end loads byte by byte.  Nothing outside
// [off, off + n) is read or written.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "e8e9_kernel.h"
#include "layout.h"

namespace zpq {

// bit k: position p + k of the block is a seed / a break; p is a multiple of kE8Lane below n
__device__ __forceinline__ E8Flags e8f_flags(const uint8_t* b, uint32_t p, uint32_t n) {
  const uint32_t have = n - p;
  uint32_t w[5] = {0u, 0u, 0u, 0u, 0u};
  if (have >= 20u) {
    uint4 v;
    __builtin_memcpy(&v, b + p, 16);
    __builtin_memcpy(&w[4], b + p + 16u, 4);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  } else {
    for (uint32_t k = 0; k < have; ++k) w[k >> 2] |= (uint32_t)b[p + k] << (8u * (k & 3u));
  }
  uint32_t t = 0, op = 0;                                       // bit k: byte p + k is 00 / ff, is e8 / e9
#pragma unroll
  for (uint32_t k = 0; k < 20u; ++k) {
    const uint32_t x = (w[k >> 2] >> (8u * (k & 3u))) & 255u;
    t |= (uint32_t)(((x + 1u) & 254u) == 0u) << k;
    op |= (uint32_t)((x & 254u) == 0xe8u) << k;
  }
  // positions p + k with k + 4 < have can be candidates; a break looks at the three behind it, up to p + 18
  const uint32_t ncand = have > 4u ? (have - 4u < 19u ? have - 4u : 19u) : 0u;
  const uint32_t cand = op & ((1u << ncand) - 1u);
  E8Flags f;
  f.seed = cand & (t >> 4) & 0xffffu;
  f.brk = cand & ~(cand >> 1) & ~(cand >> 2) & ~(cand >> 3) & 0xffffu;
  return f;
}

// (a) and (c): a workgroup of 256 per tile, as une8_mark_impl with the forward flags
template <bool kScatter>
__device__ __forceinline__ void e8f_mark_impl(const uint8_t* buf, const E8Block* blocks, uint32_t nblocks, uint32_t ntiles, uint32_t* cnt,
                                              uint32_t* status, const uint32_t* scan, uint32_t* list) {
  const uint32_t g = blockIdx.x, t = threadIdx.x & 255u;
  const uint32_t blk = une8_block_of_tile(blocks, nblocks, g);
  const E8Block B = blocks[blk];
  const uint32_t p = (g - B.tile_off) * (uint32_t)kE8Tile + t * (uint32_t)kE8Lane;
  E8Flags f;
  f.seed = 0u; f.brk = 0u;
  if (p < B.n) f = e8f_flags(buf + B.off, p, B.n);
  const uint32_t v = (uint32_t)__builtin_popcount(f.seed) | (uint32_t)__builtin_popcount(f.brk) << 16;
  uint32_t all;
  const uint32_t upto = une8_tile_scan(v, &all);
  if (!kScatter) {
    if (t == 0u) {
      cnt[g] = all & 0xffffu;
      cnt[ntiles + g] = all >> 16;
      if (g == B.tile_off) status[blk] = 0u;
      if (g == 0u) cnt[2u * ntiles] = 0u;                       // (the scan's last element: the total lands there)
    }
  } else {
    uint32_t s_at = scan[g] + ((upto - v) & 0xffffu), b_at = scan[ntiles + g] + ((upto - v) >> 16);
    for (uint32_t m = f.seed; m; m &= m - 1u) list[s_at++] = p + (uint32_t)__builtin_ctz(m);
    for (uint32_t m = f.brk; m; m &= m - 1u) list[b_at++] = p + (uint32_t)__builtin_ctz(m);
  }
}

__device__ __forceinline__ void e8f_mark_body(const uint8_t* buf, const E8Block* blocks, uint32_t nblocks, uint32_t ntiles, uint32_t* cnt,
                                              uint32_t* status) {
  e8f_mark_impl<false>(buf, blocks, nblocks, ntiles, cnt, status, nullptr, nullptr);
}
// scan: the exclusive prefix sums of cnt (2 * ntiles + 1 words: scan[ntiles] = the seeds, scan[2 * ntiles] = the list's length)
__device__ __forceinline__ void e8f_scatter_body(const uint8_t* buf, const E8Block* blocks, uint32_t nblocks, uint32_t ntiles,
                                                 const uint32_t* scan, uint32_t* list) {
  e8f_mark_impl<true>(buf, blocks, nblocks, ntiles, nullptr, nullptr, scan, list);
}

// (d) a lane per seed of the batch (nseeds = scan[ntiles] of them)
__device__ __forceinline__ void e8f_walk_body(uint8_t* buf, const E8Block* blocks, uint32_t nblocks, uint32_t ntiles, const uint32_t* scan,
                                              const uint32_t* list, uint32_t nseeds, uint32_t max_steps, uint32_t* status) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nseeds) return;
  uint32_t lo = 0, hi = nblocks;                                // the last block whose seeds start at or below q: the one that holds q
  while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (scan[blocks[mid].tile_off] <= q) lo = mid; else hi = mid; }
  const E8Block B = blocks[lo];
  const uint32_t t_end = B.tile_off + (B.n ? (uint32_t)(((uint64_t)B.n + kE8Tile - 1u) / kE8Tile) : 1u);      // (layout.h e8_tiles)
  const uint32_t s_lo = scan[B.tile_off], s_hi = scan[t_end], b_lo = scan[ntiles + B.tile_off], b_hi = scan[ntiles + t_end];
  const uint32_t s = list[q];
  uint32_t l = b_lo, h = b_hi;                                  // the first break at or above s: the top of the seed's chain
  while (l < h) { const uint32_t mid = (l + h) >> 1; if (list[mid] < s) l = mid + 1u; else h = mid; }
  if (l == b_hi) return;                                        // (a seed is a candidate: the highest candidate of a block is a break)
  if (q + 1u < s_hi && list[q + 1u] <= list[l]) return;         // the seed above belongs to the same chain: not a head
  // the lower chain's first hit rewrites the three positions above its break, which are no candidates: the walk stays above them
  const uint32_t floor = l > b_lo ? list[l - 1u] + 4u : 0u;
  uint8_t* b = buf + B.off;
  uint32_t i = s, next = q, lasthit = 0, steps = 0;             // list[next - 1]: the next lower seed, once those above i are passed
  bool live = false;                                            // a hit is at most 3 above
  for (;;) {                                                    // floor <= i, i + 4 < n
    const uint32_t x = b[i], y = b[i + 4u];
    if ((x & 254u) == 0xe8u && ((y + 1u) & 254u) == 0u) {
      const uint32_t a = ((uint32_t)b[i + 1u] | (uint32_t)b[i + 2u] << 8 | (uint32_t)b[i + 3u] << 16) + i;
      b[i + 1u] = (uint8_t)a;
      b[i + 2u] = (uint8_t)(a >> 8);
      b[i + 3u] = (uint8_t)(a >> 16);
      lasthit = i;
      live = true;
    }
    if (i <= floor) break;
    --i;
    if (!live || lasthit - i > 3u) {                            // original bytes from here on: the next hit is at the next lower seed
      live = false;
      while (next > s_lo && list[next - 1u] > i) --next;        // (the seeds passed lie in what was walked)
      if (next == s_lo) break;
      const uint32_t sn = list[next - 1u];
      if (sn < floor) break;
      i = sn;
    }
    if (++steps >= max_steps) { status[lo] = 1u; break; }
  }
}

}  // namespace zpq
