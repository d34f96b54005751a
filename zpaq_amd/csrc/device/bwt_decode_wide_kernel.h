// BWT streams of blocks of 16 MiB and more back into their blocks on the MI355X -- what the PCOMP program of the BWT methods
// computes at args[0] 5 .. 11 (host/method.cpp pcomp_bwt, arg0 > 4), for a batch of streams.  The program's count
// and link passes are those of the small form byte for byte; its walk is d = H[d]; out M[d]: the list's entry is a full 32-bit
// position, so the 24-bit limit of device/bwt_decode_kernel.h is gone and n goes up to 2^31 - 257.
//
// The stream, the order (S[b], b), the rule and the stages are those of the small decoder, whose count kernel serves both forms
// as it is (a tile's 256 words do not depend on the width of a node).  Link, the splitters' rank and emit are the small decoder's
// bodies too, over 8-byte words (BwtNode64: (uint64_t)S[b] << 32 | b, one 8-byte store of the lane that owns position b, so a step
// of either walk stays one load).  What is here:
//
//   unbwt_wide_scan_kernel     one workgroup of 1 024 per stream, thread = (part, symbol): unbwt_scan_kernel loops over all tiles of
//                              a stream twice with one wavefront per 64 symbols -- 16 384 tiles for a default block, the longest
//                              kernel of the decoder.  Here the tiles are cut into kBwtScanParts consecutive ranges: each part
//                              sums its range, the parts' sums give the totals and every part's base, the same scan over the
//                              symbols follows, and each part turns its range's counts into first nodes.  Four tiles per step, the
//                              loads in front of the stores.
//   unbwt_wide_rank2_kernel    the splitter list is ranked as the node list is: every kBwtStride2-th splitter index, and the head,
//                              is a second-level splitter.  A lane per second-level splitter walks the splitter list to the next
//                              one (splitter 0, the end, is one) and records {that one, nodes on the way, -, splitters on the way}.
//   unbwt_wide_offsets2_kernel one lane per stream follows the second-level chain from the head: n / 65 536 dependent steps where
//                              the small form makes n / 256.  Each second-level sublist on the path receives its output offset;
//                              the total is the length of the path, and anything but n declines the stream (status 1).
//   unbwt_wide_offsets1_kernel a lane per second-level splitter on the path walks its splitters again and hands each its offset.
//
// Stage boundaries are kernel boundaries; no workgroup waits for another.  Under the rule the links are injective on 1 .. n and
// nothing points to idx, so the same holds one level up: the map splitter -> next splitter is injective where it is defined,
// nothing leads to the head, the path from the head ends at entry 0 and every other walk stays on a cycle that holds its own
// start.  Every walk is bounded by the count of its level; a walk that meets an entry marked dead (its node walk ran into its
// bound) is dead itself; entries off the path keep kBwtOff as their offset and emit nothing.
//
// 32-bit arithmetic: n <= 2^31 - 257, so a position, a position + 4 095 (the end of its tile), tile * kBwtTile and
// splitter * kBwtStride stay below 2^32; sums of steps are bounded by n where the walk is live and are taken in 64 bits where a
// hostile stream could exceed that; everything that indexes the batch's arrays (link_off, out_off, in_off, g * 256) is 64-bit.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "bwt_decode_kernel.h"
#include "layout.h"

namespace zpq {

// the stream a second-level splitter belongs to: the last one whose table starts at or below g
__device__ __forceinline__ uint32_t unbwt_stream_of_splitter2(const uint32_t* sp2_off, uint32_t nstreams, uint32_t g) {
  uint32_t lo = 0, hi = nstreams;
  while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (sp2_off[mid] <= g) lo = mid; else hi = mid; }
  return lo;
}
// the splitter index of second-level splitter k of a stream whose head is splitter `head` (k >= 1)
__device__ __forceinline__ uint32_t unbwt_wide_first(uint32_t k, uint32_t head) {
  const uint32_t head2 = (head - 1u) / (uint32_t)kBwtStride2 + 1u;
  return k == head2 ? head : k * (uint32_t)kBwtStride2;
}

// (b) one workgroup of 256 * kBwtScanParts per stream, thread = (part, symbol); the tiles' counts become the tiles' first nodes, in
// place, as unbwt_scan_body leaves them
enum { kBwtScanParts = 4 };
__device__ __forceinline__ void unbwt_wide_scan_body(const BwtStream* streams, uint32_t* hist) {
  __shared__ uint32_t part[kBwtScanParts][256];
  __shared__ uint32_t sum[2][256];
  const uint32_t sym = threadIdx.x & 255u, q = (threadIdx.x >> 8) & ((uint32_t)kBwtScanParts - 1u);
  const BwtStream S = streams[blockIdx.x];
  const uint32_t ntiles = (S.n + (uint32_t)kBwtTile) / (uint32_t)kBwtTile;
  const uint32_t per = (ntiles + (uint32_t)kBwtScanParts - 1u) / (uint32_t)kBwtScanParts;
  const uint32_t t0 = q * per < ntiles ? q * per : ntiles, t1 = t0 + per < ntiles ? t0 + per : ntiles;
  uint32_t* h = hist + (uint64_t)S.tile_off * 256u + sym;
  uint32_t mine = 0, t = t0;
  for (; t + 4u <= t1; t += 4u) {
    const uint32_t c0 = h[(uint64_t)t * 256u], c1 = h[(uint64_t)(t + 1u) * 256u], c2 = h[(uint64_t)(t + 2u) * 256u], c3 = h[(uint64_t)(t + 3u) * 256u];
    mine += c0 + c1 + c2 + c3;
  }
  for (; t < t1; ++t) mine += h[(uint64_t)t * 256u];
  part[q][sym] = mine;
  __syncthreads();
  uint32_t total = 0, before = 0;
  for (uint32_t k = 0; k < (uint32_t)kBwtScanParts; ++k) { const uint32_t v = part[k][sym]; total += v; if (k < q) before += v; }
  uint32_t cur = 0;
  if (q == 0u) sum[0][sym] = total;
  __syncthreads();
  for (uint32_t d = 1; d < 256u; d <<= 1) {                     // inclusive scan by part 0: read one buffer, write the other
    if (q == 0u) sum[cur ^ 1u][sym] = sum[cur][sym] + (sym >= d ? sum[cur][sym - d] : 0u);
    __syncthreads();
    cur ^= 1u;
  }
  uint32_t run = 1u + sum[cur][sym] - total + before;
  for (t = t0; t + 4u <= t1; t += 4u) {
    const uint32_t c0 = h[(uint64_t)t * 256u], c1 = h[(uint64_t)(t + 1u) * 256u], c2 = h[(uint64_t)(t + 2u) * 256u], c3 = h[(uint64_t)(t + 3u) * 256u];
    h[(uint64_t)t * 256u] = run;
    h[(uint64_t)(t + 1u) * 256u] = run + c0;
    h[(uint64_t)(t + 2u) * 256u] = run + c0 + c1;
    h[(uint64_t)(t + 3u) * 256u] = run + c0 + c1 + c2;
    run += c0 + c1 + c2 + c3;
  }
  for (; t < t1; ++t) {
    const uint32_t c = h[(uint64_t)t * 256u];
    h[(uint64_t)t * 256u] = run;
    run += c;
  }
}

// (e1) a lane per second-level splitter of the batch (nsplit2 of them); sp2: {next second-level splitter, nodes, output offset, splitters}
__device__ __forceinline__ void unbwt_wide_rank2_body(const BwtStream* streams, const uint32_t* sp2_off, uint32_t nstreams, uint32_t nsplit2,
                                                      const uint4* sp_all, uint4* sp2) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nsplit2) return;
  const uint32_t b = unbwt_stream_of_splitter2(sp2_off, nstreams, g);
  const BwtStream S = streams[b];
  const uint32_t k = g - sp2_off[b], head = S.n / (uint32_t)kBwtStride + 1u;
  uint4 r;
  r.x = 0u; r.y = 0u; r.z = kBwtOff; r.w = 0u;
  if (k) {
    const uint4* sp = sp_all + S.sp_off;
    uint32_t j = unbwt_wide_first(k, head), hops = 0;
    uint64_t nodes = 0;
    bool dead = false;
    do {
      const uint4 e = sp[j];
      nodes += e.y;
      ++hops;
      if (e.x == kBwtOff || e.x >= head || nodes > S.n) { dead = true; break; }
      j = e.x;
    } while ((j & ((uint32_t)kBwtStride2 - 1u)) && hops <= head);
    if (!dead && (j & ((uint32_t)kBwtStride2 - 1u))) dead = true;
    r.x = dead ? kBwtOff : j / (uint32_t)kBwtStride2;
    r.y = dead ? 0u : (uint32_t)nodes;
    r.w = hops;
  }
  sp2[g] = r;
}

// (e2) one lane per stream (64 threads per workgroup, lane 0 works); status[b]: 0 the path has n nodes, 1 declined
__device__ __forceinline__ void unbwt_wide_offsets2_body(const BwtStream* streams, const uint32_t* sp2_off, uint4* sp2_all, uint32_t* status) {
  if ((threadIdx.x & 63u) != 0u) return;
  const BwtStream S = streams[blockIdx.x];
  uint4* sp2 = sp2_all + sp2_off[blockIdx.x];
  const uint32_t head = S.n / (uint32_t)kBwtStride + 1u, head2 = (head - 1u) / (uint32_t)kBwtStride2 + 1u;
  uint32_t k = head2, hops = 0;
  uint64_t off = 0;
  bool ok = true;
  for (;;) {
    const uint4 e = sp2[k];
    if (e.x == kBwtOff) { ok = false; break; }
    sp2[k].z = (uint32_t)off;
    off += e.y;
    if (e.x == 0u) break;                                       // splitter 0 is node 0: the end
    if (e.x >= head2 || ++hops > head2 || off > S.n) { ok = false; break; }
    k = e.x;
  }
  status[blockIdx.x] = ok && off == S.n ? 0u : 1u;
}

// (e3) a lane per second-level splitter of the batch: the splitters of its sublist receive their offsets
__device__ __forceinline__ void unbwt_wide_offsets1_body(const BwtStream* streams, const uint32_t* sp2_off, uint32_t nstreams, uint32_t nsplit2,
                                                         uint4* sp_all, const uint4* sp2, const uint32_t* status) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nsplit2) return;
  const uint32_t b = unbwt_stream_of_splitter2(sp2_off, nstreams, g);
  if (status[b] != 0u) return;
  const BwtStream S = streams[b];
  const uint32_t k = g - sp2_off[b], head = S.n / (uint32_t)kBwtStride + 1u;
  const uint4 e2 = sp2[g];
  if (!k || e2.z == kBwtOff || e2.x == kBwtOff) return;
  uint4* sp = sp_all + S.sp_off;
  uint32_t j = unbwt_wide_first(k, head), off = e2.z;
  for (uint32_t h = 0; h < e2.w; ++h) {
    const uint4 e = sp[j];
    sp[j].z = off;
    off += e.y;
    j = e.x;
  }
}

// (c), (d), (f): the small decoder's bodies, which take the form from the list's word.  The names they had as bodies of their own,
// for sources written against those
__device__ __forceinline__ void unbwt_wide_link_body(const uint8_t* in_all, const BwtStream* streams, uint32_t nstreams, const uint32_t* hist,
                                                     uint64_t* link_all) {
  unbwt_link_body(in_all, streams, nstreams, hist, link_all);
}
__device__ __forceinline__ void unbwt_wide_rank_body(const BwtStream* streams, uint32_t nstreams, uint32_t nsplit, const uint64_t* link_all, uint4* sp) {
  unbwt_rank_body(streams, nstreams, nsplit, link_all, sp);
}
__device__ __forceinline__ void unbwt_wide_emit_body(const BwtStream* streams, uint32_t nstreams, uint32_t nsplit, const uint64_t* link_all,
                                                     const uint4* sp, const uint32_t* status, uint8_t* out_all) {
  unbwt_emit_body(streams, nstreams, nsplit, link_all, sp, status, out_all);
}

}  // namespace zpq
