// BWT streams back into their blocks on the MI355X -- what the PCOMP program of the BWT methods without E8E9 computes at
// args[0] <= 4 (host/method.cpp pcomp_bwt, run by host/postproc.cpp), for a batch of streams.  A stream is S[0 .. n] and idx in
// 4 bytes, low byte first; S[idx] == 255 is the marker and no byte of the block.
//
// The program counts the bytes, links every position b != idx into a list ordered by (S[b], b) -- node r + 1 points to the r-th
// position of that order -- and walks the list from idx to node 0, emitting the byte of every node it arrives at.  Neither half
// is byte-serial: the order is one stable 8-bit counting sort, and a list can be walked from many nodes at once.
//
//   unbwt_count_kernel    one wavefront per tile of kBwtTile positions: a 256-bin histogram in LDS (ds_add), b == idx skipped,
//                         written out as the tile's 256 words.
//   unbwt_scan_kernel     one workgroup of 256 per stream, lane = symbol: the sum over the tiles, an exclusive scan over the
//                         symbols, then the tile's word becomes the first node of (symbol, tile):
//                         1 + #(bytes < symbol) + #(symbol in earlier tiles).
//   unbwt_link_kernel     one wavefront per tile, 64 positions at a time in order: eight ballots over the byte's bits give the
//                         lanes with an equal byte, the rank among the lower ones places the lane, the group's highest lane adds
//                         the group's size to the symbol's counter in LDS.  Equal bytes keep their order: that is what makes the
//                         list the program's.  Node p's word holds b and S[b]: where the walk goes and what it emits there, so
//                         a step is one load.
//   unbwt_rank_kernel     a lane per splitter -- every kBwtStride-th node, and the head idx -- walks to the next splitter (node 0,
//                         the end, is one) and records {that splitter, steps}.
//   unbwt_offsets_kernel  one lane per stream follows the splitters from the head: n / kBwtStride dependent steps over a table
//                         that stays in L2.  Each sublist on the path receives its output offset; the total is the length of the
//                         path, and anything but n declines the stream (status 1).
//   unbwt_emit_kernel     a lane per splitter on the path walks again and writes out[offset .. offset + steps), four bytes
//                         gathered into an aligned word where the word lies inside the range.  No lane writes outside its own
//                         sublist's range, so the result does not depend on the order of lanes.
//
// Stage boundaries are kernel boundaries; no workgroup waits for another.  Under the rule (1 <= idx <= n, S[idx] == 255, checked
// by the caller: layout.h bwt_stream_admitted) the links are injective on 1 .. n and nothing points to idx, so the path from idx
// ends at node 0 and every other walk stays on a cycle that holds its own start: every walk is bounded by n steps, whatever the
// bytes.  Bytes that are no BWT may leave cycles beside the path; the path is then shorter than n and the stream is declined.
//
// Link, rank and emit are templates over the node's word (BwtNode32 here, BwtNode64 for device/bwt_decode_wide_kernel.h): how b
// and S[b] are packed into it is all that the two forms' lists differ in.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "layout.h"

namespace zpq {

static const uint32_t kBwtOff = 0xFFFFFFFFu;        // a splitter's next: dead; its offset: not on the path

// A node's word, by its type: the position the walk goes to and the byte it emits there.  Link, rank and emit take the form
// from the type of the list they are given.  4 bytes, b << 8 | S[b]: positions below 2^24.
template <class Word> struct BwtNode;
template <> struct BwtNode<uint32_t> {
  static __device__ __forceinline__ uint32_t pack(uint32_t node, uint32_t v) { return node << 8 | v; }
  static __device__ __forceinline__ uint32_t next(uint32_t w) { return w >> 8; }
  static __device__ __forceinline__ uint32_t byte(uint32_t w) { return w & 255u; }
};
// 8 bytes, (uint64_t)S[b] << 32 | b: a full 32-bit position, one 8-byte store of the lane that owns position b
template <> struct BwtNode<uint64_t> {
  static __device__ __forceinline__ uint64_t pack(uint32_t node, uint32_t v) { return (uint64_t)v << 32 | node; }
  static __device__ __forceinline__ uint32_t next(uint64_t w) { return (uint32_t)w; }
  static __device__ __forceinline__ uint32_t byte(uint64_t w) { return (uint32_t)(w >> 32) & 255u; }
};
typedef BwtNode<uint32_t> BwtNode32;
typedef BwtNode<uint64_t> BwtNode64;

// the stream a tile / a splitter belongs to: the last one that starts at or below g (every stream has some of each)
__device__ __forceinline__ uint32_t unbwt_stream_of_tile(const BwtStream* streams, uint32_t nstreams, uint32_t g) {
  uint32_t lo = 0, hi = nstreams;
  while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (streams[mid].tile_off <= g) lo = mid; else hi = mid; }
  return lo;
}
__device__ __forceinline__ uint32_t unbwt_stream_of_splitter(const BwtStream* streams, uint32_t nstreams, uint32_t g) {
  uint32_t lo = 0, hi = nstreams;
  while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (streams[mid].sp_off <= g) lo = mid; else hi = mid; }
  return lo;
}

// (a) one wavefront per tile (64 threads per workgroup); hist: 256 words per tile
__device__ __forceinline__ void unbwt_count_body(const uint8_t* in_all, const BwtStream* streams, uint32_t nstreams, uint32_t* hist) {
  __shared__ uint32_t bins[256];
  const uint32_t g = blockIdx.x, lane = threadIdx.x & 63u;
  const BwtStream S = streams[unbwt_stream_of_tile(streams, nstreams, g)];
  const uint32_t first = (g - S.tile_off) * (uint32_t)kBwtTile;
  const uint32_t* words = (const uint32_t*)(in_all + S.in_off) + first / 4u;        // (the stream goes on for 4 bytes behind S[n])
  for (uint32_t k = 0; k < 4u; ++k) bins[lane + 64u * k] = 0u;
  __syncthreads();
  for (uint32_t i = 0; i < (uint32_t)kBwtTile / 256u; ++i) {
    const uint32_t at = first + 4u * (i * 64u + lane);
    if (at > S.n) break;
    const uint32_t w = words[i * 64u + lane];
    for (uint32_t k = 0; k < 4u; ++k) {
      const uint32_t p = at + k;
      if (p <= S.n && p != S.idx) atomicAdd(&bins[(w >> (8u * k)) & 255u], 1u);
    }
  }
  __syncthreads();
  for (uint32_t k = 0; k < 4u; ++k) hist[(uint64_t)g * 256u + lane + 64u * k] = bins[lane + 64u * k];
}

// (b) one workgroup of 256 per stream, thread = symbol; the tiles' counts become the tiles' first nodes, in place
__device__ __forceinline__ void unbwt_scan_body(const BwtStream* streams, uint32_t* hist) {
  __shared__ uint32_t sum[2][256];
  const uint32_t sym = threadIdx.x & 255u;
  const BwtStream S = streams[blockIdx.x];
  const uint32_t ntiles = (S.n + (uint32_t)kBwtTile) / (uint32_t)kBwtTile;
  uint32_t* h = hist + (uint64_t)S.tile_off * 256u + sym;
  uint32_t total = 0;
  for (uint32_t t = 0; t < ntiles; ++t) total += h[(uint64_t)t * 256u];
  uint32_t cur = 0;
  sum[0][sym] = total;
  __syncthreads();
  for (uint32_t d = 1; d < 256u; d <<= 1) {                     // inclusive scan: read one buffer, write the other
    const uint32_t v = sum[cur][sym] + (sym >= d ? sum[cur][sym - d] : 0u);
    sum[cur ^ 1u][sym] = v;
    __syncthreads();
    cur ^= 1u;
  }
  uint32_t run = 1u + sum[cur][sym] - total;
  for (uint32_t t = 0; t < ntiles; ++t) {
    const uint32_t c = h[(uint64_t)t * 256u];
    h[(uint64_t)t * 256u] = run;
    run += c;
  }
}

// (c) one wavefront per tile (64 threads per workgroup); link: node p of stream b at link_all[link_off + p]
template <class Word>
__device__ __forceinline__ void unbwt_link_body(const uint8_t* in_all, const BwtStream* streams, uint32_t nstreams, const uint32_t* hist,
                                                Word* link_all) {
  __shared__ uint32_t base[256];
  const uint32_t g = blockIdx.x, lane = threadIdx.x & 63u;
  const BwtStream S = streams[unbwt_stream_of_tile(streams, nstreams, g)];
  const uint32_t first = (g - S.tile_off) * (uint32_t)kBwtTile;
  const uint8_t* s = in_all + S.in_off;
  Word* link = link_all + S.link_off;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (uint32_t k = 0; k < 4u; ++k) base[lane + 64u * k] = hist[(uint64_t)g * 256u + lane + 64u * k];
  __syncthreads();
  for (uint32_t c = 0; c < (uint32_t)kBwtTile / (uint32_t)kBwtChunk; ++c) {
    const uint32_t p0 = first + c * (uint32_t)kBwtChunk;
    if (p0 > S.n) break;                                        // (the same in every lane)
    const uint32_t node = p0 + lane;
    const bool live = node <= S.n && node != S.idx;
    const uint32_t v = node <= S.n ? s[node] : 0u;
    unsigned long long same = __builtin_amdgcn_ballot_w64(live);
    for (uint32_t k = 0; k < 8u; ++k) {
      const bool bit = (v >> k) & 1u;
      const unsigned long long m = __builtin_amdgcn_ballot_w64(bit);
      same &= bit ? m : ~m;
    }
    const uint32_t rank = (uint32_t)__builtin_popcountll(same & below), size = (uint32_t)__builtin_popcountll(same);
    if (live) link[base[v] + rank] = BwtNode<Word>::pack(node, v);
    __syncthreads();                                            // (every lane has read its counter)
    if (live && rank + 1u == size) base[v] += size;
    __syncthreads();
  }
}

// (d) a lane per splitter of the batch (nsplit of them); sp: {next splitter, steps, output offset, -}
template <class Word>
__device__ __forceinline__ void unbwt_rank_body(const BwtStream* streams, uint32_t nstreams, uint32_t nsplit, const Word* link_all,
                                                uint4* sp) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nsplit) return;
  const BwtStream S = streams[unbwt_stream_of_splitter(streams, nstreams, g)];
  const uint32_t j = g - S.sp_off, head = S.n / (uint32_t)kBwtStride + 1u;
  uint4 r;
  r.x = 0u; r.y = 0u; r.z = kBwtOff; r.w = 0u;                  // z: not on the path, until the offsets say otherwise
  if (j) {
    const Word* link = link_all + S.link_off;
    uint32_t d = j == head ? S.idx : j * (uint32_t)kBwtStride, steps = 0;
    do { d = BwtNode<Word>::next(link[d]); ++steps; } while ((d & ((uint32_t)kBwtStride - 1u)) && steps < S.n);
    r.x = (d & ((uint32_t)kBwtStride - 1u)) ? kBwtOff : d / (uint32_t)kBwtStride;
    r.y = steps;
  }
  sp[g] = r;
}

// (e) one lane per stream (64 threads per workgroup, lane 0 works); status[b]: 0 the path has n nodes, 1 declined
__device__ __forceinline__ void unbwt_offsets_body(const BwtStream* streams, uint4* sp_all, uint32_t* status) {
  if ((threadIdx.x & 63u) != 0u) return;
  const BwtStream S = streams[blockIdx.x];
  uint4* sp = sp_all + S.sp_off;
  const uint32_t head = S.n / (uint32_t)kBwtStride + 1u;
  uint32_t j = head, off = 0, hops = 0;
  bool ok = true;
  for (;;) {
    const uint4 e = sp[j];
    sp[j].z = off;
    off += e.y;
    if (e.x == 0u) break;                                       // node 0: the end
    if (e.x >= head || ++hops > head || off > S.n) { ok = false; break; }
    j = e.x;
  }
  status[blockIdx.x] = ok && off == S.n ? 0u : 1u;
}

// the bytes a lane holds for one aligned word of the output, [from, to) with to - from <= 4
__device__ __forceinline__ void unbwt_flush(uint8_t* out, uint64_t from, uint64_t to, uint32_t acc) {
  if (to - from == 4u) { *(uint32_t*)(out + from) = acc; return; }
  for (uint64_t q = from; q < to; ++q) out[q] = (uint8_t)(acc >> (8u * (uint32_t)((uintptr_t)(out + q) & 3u)));
}

// (f) a lane per splitter of the batch; stream b's output at out_all + out_off
template <class Word>
__device__ __forceinline__ void unbwt_emit_body(const BwtStream* streams, uint32_t nstreams, uint32_t nsplit, const Word* link_all,
                                                const uint4* sp, const uint32_t* status, uint8_t* out_all) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nsplit) return;
  const uint32_t b = unbwt_stream_of_splitter(streams, nstreams, g);
  if (status[b] != 0u) return;
  const BwtStream S = streams[b];
  const uint32_t j = g - S.sp_off, head = S.n / (uint32_t)kBwtStride + 1u;
  const uint4 e = sp[g];
  if (!j || e.z == kBwtOff) return;
  const Word* link = link_all + S.link_off;
  uint8_t* out = out_all;
  uint64_t pos = S.out_off + e.z, from = pos;
  uint32_t d = j == head ? S.idx : j * (uint32_t)kBwtStride, acc = 0;
  for (uint32_t k = 0; k < e.y; ++k) {
    const Word w = link[d];
    d = BwtNode<Word>::next(w);
    acc |= BwtNode<Word>::byte(w) << (8u * (uint32_t)((uintptr_t)(out + pos) & 3u));
    ++pos;
    if (((uintptr_t)(out + pos) & 3u) == 0u) { unbwt_flush(out, from, pos, acc); acc = 0u; from = pos; }
  }
  if (from < pos) unbwt_flush(out, from, pos, acc);
}

}  // namespace zpq
