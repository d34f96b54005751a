// The inverse E8E9 filter on the MI355X -- what kE8Loop / kPcompE8 of host/method.cpp and e8e9_inverse of host/preproc.cpp
// compute, for a batch of blocks that lie in one device buffer, in place.  The scan looks byte-serial: at position i it tests
// (b[i] & 254) == 0xe8 and ((b[i + 4] + 1) & 254) == 0, a hit rewrites b[i + 1 .. i + 3] (the address minus i, mod 2^24), and a
// rewritten byte can make or unmake the next opcode.  It is serial only along short chains:
//
//   - a hit at j writes j + 1 .. j + 3 and only j < i ran when i is visited, so b[i + 4] is still original there:
//     cand(i) = i + 4 < n && orig[i + 4] in {00, ff} is known for every position at once;
//   - only a hit at i - 3 .. i - 1 can change what i sees.  A BREAK is a candidate with no candidate in the three positions in
//     front of it; a CHAIN runs from a break to the last candidate in front of the next break.  Chains neither read nor write
//     each other's bytes, given that a walk stops three positions in front of the next break (those are no candidates);
//   - a SEED is a candidate whose original byte is e8 / e9.  More than three positions behind its last hit a walk sees original
//     bytes only, so the next possible hit is the next seed, and a chain without a seed has no hit.
//
//   une8_mark_kernel      a lane per 16 bytes (one 16-byte load and a word), a workgroup of 256 per tile of kE8Tile bytes: the
//                         seed and break flags of the lane's positions, their counts summed over the tile -> cnt[tile],
//                         cnt[ntiles + tile]; status[block] = 0.
//   -- an exclusive scan over the 2 * ntiles + 1 counts (rocPRIM); the host reads the two totals and sizes the list --
//   une8_scatter_kernel   the same flags again (the bytes are still original) and a prefix over the workgroup's lanes: the
//                         positions of the seeds, then of the breaks, into one list, sorted per block.
//   une8_walk_kernel      a lane per seed.  A seed is a HEAD when a break lies in (previous seed, seed]: one binary search; the
//                         others leave.  A head tests and rewrites position by position while a hit is at most 3 behind, else
//                         jumps to the next seed, and ends when that lies at or behind the next break.  The rewritten bytes go
//                         out as byte stores: neighbouring chains may share a word.  After max_steps steps a lane gives up and
//                         sets status[block] = 1: the block is declined and nothing of it may be delivered.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "layout.h"

namespace zpq {

// the block a tile belongs to: the last one that starts at or below g (every block has a tile)
__device__ __forceinline__ uint32_t une8_block_of_tile(const E8Block* blocks, uint32_t nblocks, uint32_t g) {
  uint32_t lo = 0, hi = nblocks;
  while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (blocks[mid].tile_off <= g) lo = mid; else hi = mid; }
  return lo;
}

// bit k: position p + k of the block is a seed / a break; p is a multiple of kE8Lane below n
struct E8Flags { uint32_t seed, brk; };
__device__ __forceinline__ E8Flags une8_flags(const uint8_t* b, uint32_t p, uint32_t n) {
  const uint4 v = *(const uint4*)(b + p);                       // (the room behind a block is rounded up to 16)
  const uint32_t w[5] = {v.x, v.y, v.z, v.w, p + 16u < n ? *(const uint32_t*)(b + p + 16u) : 0u};
  uint32_t t = 0, op = 0;                                       // bit k: byte p + k is 00 / ff, is e8 / e9
#pragma unroll
  for (uint32_t k = 0; k < 20u; ++k) {
    const uint32_t x = (w[k >> 2] >> (8u * (k & 3u))) & 255u;
    t |= (uint32_t)(((x + 1u) & 254u) == 0u) << k;
    op |= (uint32_t)((x & 254u) == 0xe8u) << k;
  }
  const uint32_t have = n - p;                                  // positions p + k with k + 4 < have can be candidates
  const uint32_t ncand = have > 4u ? (have - 4u < 16u ? have - 4u : 16u) : 0u;
  const uint32_t cand = (t >> 4) & ((1u << ncand) - 1u);
  // the three positions in front of p: p - 3 + j is a candidate when byte p + 1 + j is 00 / ff and lies in the block
  const uint32_t nprior = have - 1u < 3u ? have - 1u : 3u;
  const uint32_t prior = p ? (t >> 1) & ((1u << nprior) - 1u) : 0u;
  const uint32_t e = prior | cand << 3;
  E8Flags f;
  f.seed = cand & op & 0xffffu;
  f.brk = (e >> 3) & ~(e >> 2) & ~(e >> 1) & ~e & 0xffffu;
  return f;
}

// inclusive prefix of v over the workgroup's 256 lanes, *all = the sum; every lane of the workgroup calls it
__device__ __forceinline__ uint32_t une8_tile_scan(uint32_t v, uint32_t* all) {
  __shared__ uint32_t wave_sum[4];
  const uint32_t lane = threadIdx.x & 63u, wave = (threadIdx.x >> 6) & 3u;
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const uint32_t o = __shfl(v, (int)((lane - d) & 63u));
    if (lane >= d) v += o;
  }
  if (lane == 63u) wave_sum[wave] = v;
  __syncthreads();
  uint32_t before = 0, sum = 0;
  for (uint32_t k = 0; k < 4u; ++k) {
    const uint32_t s = wave_sum[k];
    if (k < wave) before += s;
    sum += s;
  }
  *all = sum;
  return v + before;
}

// (a) and (c): a workgroup of 256 per tile.  kScatter = false: the tile's counts and the blocks' statuses; true: the positions into
// `list` from where the scanned counts say.  A tile holds at most 4 096 of either: seeds in the low half of a word, breaks above.
template <bool kScatter>
__device__ __forceinline__ void une8_mark_impl(const uint8_t* buf, const E8Block* blocks, uint32_t nblocks, uint32_t ntiles, uint32_t* cnt,
                                               uint32_t* status, const uint32_t* scan, uint32_t* list) {
  const uint32_t g = blockIdx.x, t = threadIdx.x & 255u;
  const uint32_t blk = une8_block_of_tile(blocks, nblocks, g);
  const E8Block B = blocks[blk];
  const uint32_t p = (g - B.tile_off) * (uint32_t)kE8Tile + t * (uint32_t)kE8Lane;
  E8Flags f;
  f.seed = 0u; f.brk = 0u;
  if (p < B.n) f = une8_flags(buf + B.off, p, B.n);
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

__device__ __forceinline__ void une8_mark_body(const uint8_t* buf, const E8Block* blocks, uint32_t nblocks, uint32_t ntiles, uint32_t* cnt,
                                               uint32_t* status) {
  une8_mark_impl<false>(buf, blocks, nblocks, ntiles, cnt, status, nullptr, nullptr);
}
// scan: the exclusive prefix sums of cnt (2 * ntiles + 1 words: scan[ntiles] = the seeds, scan[2 * ntiles] = the list's length)
__device__ __forceinline__ void une8_scatter_body(const uint8_t* buf, const E8Block* blocks, uint32_t nblocks, uint32_t ntiles,
                                                  const uint32_t* scan, uint32_t* list) {
  une8_mark_impl<true>(buf, blocks, nblocks, ntiles, nullptr, nullptr, scan, list);
}

// (d) a lane per seed of the batch (nseeds = scan[ntiles] of them)
__device__ __forceinline__ void une8_walk_body(uint8_t* buf, const E8Block* blocks, uint32_t nblocks, uint32_t ntiles, const uint32_t* scan,
                                               const uint32_t* list, uint32_t nseeds, uint32_t max_steps, uint32_t* status) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nseeds) return;
  uint32_t lo = 0, hi = nblocks;                                // the last block whose seeds start at or below q: the one that holds q
  while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (scan[blocks[mid].tile_off] <= q) lo = mid; else hi = mid; }
  const E8Block B = blocks[lo];
  const uint32_t t_end = B.tile_off + (B.n ? (uint32_t)(((uint64_t)B.n + kE8Tile - 1u) / kE8Tile) : 1u);      // (layout.h e8_tiles)
  const uint32_t s_lo = scan[B.tile_off], s_hi = scan[t_end], b_lo = scan[ntiles + B.tile_off], b_hi = scan[ntiles + t_end];
  const uint32_t s = list[q];
  uint32_t l = b_lo, h = b_hi;                                  // the first break behind s
  while (l < h) { const uint32_t mid = (l + h) >> 1; if (list[mid] <= s) l = mid + 1u; else h = mid; }
  if (l == b_lo) return;                                        // (a seed is a candidate: its chain's break is at or below it)
  if (q > s_lo && list[l - 1u] <= list[q - 1u]) return;         // the seed in front belongs to the same chain: not a head
  const uint32_t n = B.n;
  const uint32_t end = l < b_hi ? list[l] : 0xFFFFFFFFu;        // the next chain's break
  // positions end - 3 .. end - 1 are no candidates and the next chain may rewrite what lies 4 behind them: the walk stays below
  const uint32_t lim = l < b_hi && end - 3u < n - 4u ? end - 3u : n - 4u;
  uint8_t* b = buf + B.off;
  uint32_t i = s, next = q + 1u, lasthit = 0, steps = 0;
  bool live = false;                                            // a hit is at most 3 behind
  for (;;) {                                                    // i < lim
    const uint32_t x = b[i], y = b[i + 4u];
    if ((x & 254u) == 0xe8u && ((y + 1u) & 254u) == 0u) {
      const uint32_t a = ((uint32_t)b[i + 1u] | (uint32_t)b[i + 2u] << 8 | (uint32_t)b[i + 3u] << 16) - i;
      b[i + 1u] = (uint8_t)a;
      b[i + 2u] = (uint8_t)(a >> 8);
      b[i + 3u] = (uint8_t)(a >> 16);
      lasthit = i;
      live = true;
    }
    ++i;
    if (!live || i - lasthit > 3u) {                            // original bytes from here on: the next hit is at the next seed
      live = false;
      while (next < s_hi && list[next] < i) ++next;             // (the seeds passed lie in what was walked)
      if (next >= s_hi) break;
      const uint32_t sn = list[next];
      if (sn >= end) break;
      i = sn;
    }
    if (i >= lim) break;
    if (++steps >= max_steps) { status[lo] = 1u; break; }
  }
}

}  // namespace zpq
