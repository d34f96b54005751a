// Suffix arrays of many blocks at once on the MI355X -- the sort behind compressBlock's byte-aligned LZ77 and BWT
// pre-processors (LZBuffer with a suffix array, libzpaq.cpp:6463-6883; divsufsort / divbwt, 4658-6434).  A suffix array
// is canonical, so any correct builder gives the reference's parse and the reference's BWT; divsufsort's induced sorting
// is a serial algorithm, this is prefix doubling (Manber-Myers / Larsson-Sadakane) laid out for a GPU:
//
//   every suffix of every block is one element of ONE array (block b owns [off_b, off_b + n_b)); round h sorts all
//   elements by the 64-bit key  block << 48 | rank_h[i] << 24 | rank_h[i + h]  (rank 0 = past the end of the block: the
//   end of the string sorts before every byte, as in the reference) with one radix sort, then renames: equal neighbours
//   keep a rank, a flag + prefix sum gives the others theirs, relative to the block's first element.  After the round
//   ranks order the suffixes by their first 2h bytes; when every key of a round is distinct the ranks are the inverse
//   suffix array.  log2(longest repeat) rounds: 3-4 for random data, 6-8 for text, log2(n) for a block of zeros.
//   The kernels' bodies and the loop's two decisions are in device/sa_kernel.h (the emulator runs them: tests/emu/sa_emu_main.cpp).
//
// Each round streams the arrays a few times at HBM rate (radix sort of 64-bit keys + 32-bit values, one gather, one
// scan, one scatter): bandwidth work, no MFMA.  Blocks below 2^24 bytes and 65 535 blocks per call; a block of 2^24 bytes
// and more is sorted alone by the wide sorter below (device/sa_wide_kernel.h: no block id, rank fields of up to 31 bits); the
// caller (host/blocks.cpp) keeps the host's SA-IS for small batches and for what the device declines.
#include <hip/hip_runtime.h>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <cstdint>

#include "bwt_decode_kernel.h"
#include "bwt_decode_wide_kernel.h"
#include "e8e9_forward_kernel.h"
#include "e8e9_kernel.h"
#include "fragment_kernel.h"
#include "lz77_codes_kernel.h"
#include "lz77_decode_kernel.h"
#include "lz77_decode_wide_kernel.h"
#include "lz77_hash_kernel.h"
#include "lz77_kernel.h"
#include "lz77_wide_kernel.h"
#include "sa_kernel.h"
#include "sa_kernels.h"
#include "sa_wide_kernel.h"

namespace zpq {

namespace {

__global__ __launch_bounds__(256) void sa_init_kernel(const uint8_t* const* in, const uint64_t* off, uint32_t nblocks, uint64_t total,
                                                      uint32_t* rank, uint16_t* blk) {
  sa_init_body(in, off, nblocks, total, rank, blk);
}
__global__ __launch_bounds__(256) void sa_keys_kernel(const uint32_t* rank, const uint16_t* blk, const uint64_t* off, uint64_t total, uint32_t h,
                                                      uint64_t* keys, uint32_t* vals) {
  sa_keys_body(rank, blk, off, total, h, keys, vals);
}
__global__ __launch_bounds__(256) void sa_flags_kernel(const uint64_t* keys, uint64_t total, uint32_t* flags) { sa_flags_body(keys, total, flags); }
__global__ __launch_bounds__(256) void sa_rename_kernel(const uint64_t* keys, const uint32_t* vals, const uint32_t* scan, const uint64_t* off,
                                                        uint64_t total, uint32_t* rank) {
  sa_rename_body(keys, vals, scan, off, total, rank);
}
__global__ __launch_bounds__(256) void sa_invert_kernel(const uint32_t* rank, const uint16_t* blk, const uint64_t* off, uint64_t total, uint32_t* sa) {
  sa_invert_body(rank, blk, off, total, sa);
}

inline unsigned grid_for(uint64_t n) { return (unsigned)((n + 255) / 256); }

__global__ __launch_bounds__(256) void sa_wide_init_kernel(const uint8_t* in, uint32_t n, uint32_t* rank) { sa_wide_init_body(in, n, rank); }
__global__ __launch_bounds__(256) void sa_wide_keys_kernel(const uint32_t* rank, uint32_t n, uint32_t h, uint32_t w, uint64_t* keys, uint32_t* vals) {
  sa_wide_keys_body(rank, n, h, w, keys, vals);
}
__global__ __launch_bounds__(256) void sa_wide_rename_kernel(const uint32_t* vals, const uint32_t* scan, uint32_t n, uint32_t* rank) {
  sa_wide_rename_body(vals, scan, n, rank);
}
__global__ __launch_bounds__(256) void sa_wide_invert_kernel(const uint32_t* rank, uint32_t n, uint32_t* sa) { sa_wide_invert_body(rank, n, sa); }
__global__ __launch_bounds__(256) void bwt_wide_kernel(const uint8_t* in, const uint32_t* rank, uint32_t n, uint8_t* out, uint32_t* idx) {
  bwt_wide_body(in, rank, n, out, idx);
}

__global__ __launch_bounds__(256) void lz77_search_kernel(const uint8_t* in_all, const uint32_t* sa_all, const uint32_t* rank_all, const uint16_t* blk,
                                                          const LzBlock* blocks, uint64_t total, uint4* res) {
  lz77_search_body(in_all, sa_all, rank_all, blk, blocks, total, res);
}
__global__ __launch_bounds__(64) void lz77_walk_kernel(const LzBlock* blocks, const uint4* res, LzTok* toks, uint32_t* counts) {
  lz77_walk_body(blocks, res, toks, counts);
}
// device/lz77_wide_kernel.h: the parse of one block of any length below 2^31 in pieces
__global__ __launch_bounds__(256) void lz77_wide_search_kernel(const uint8_t* in, const uint32_t* sa, const uint32_t* rank, const LzBlock* blocks, uint4* res) {
  lz77_wide_search_body(in, sa, rank, blocks, res);
}
__global__ __launch_bounds__(64) void lz77_wide_walk_kernel(LzWideParams W, const uint4* res, LzTok* prov, LzWidePiece* pieces) {
  lz77_wide_walk_body(W, res, prov, pieces);
}
__global__ __launch_bounds__(64) void lz77_wide_stitch_kernel(LzWideParams W, const uint4* res, const LzTok* prov, const LzWidePiece* pieces, LzTok* toks,
                                                              uint32_t tok_cap, LzWideAdopt* adopt, LzWideResult* out) {
  lz77_wide_stitch_body(W, res, prov, pieces, toks, tok_cap, adopt, out);
}
__global__ __launch_bounds__(256) void lz77_wide_gather_kernel(LzWideParams W, const LzTok* prov, const LzWideAdopt* adopt, LzTok* toks, uint32_t tok_cap) {
  lz77_wide_gather_body(W, prov, adopt, toks, tok_cap);
}
__global__ __launch_bounds__(256) void bwt_emit_kernel(const uint8_t* in_all, const uint32_t* sa_all, const uint16_t* blk, const LzBlock* blocks,
                                                       uint64_t total, uint8_t* out_all, uint32_t* idx) {
  bwt_emit_body(in_all, sa_all, blk, blocks, total, out_all, idx);
}

__global__ __launch_bounds__(256) void lzh_keys_kernel(const uint8_t* in_all, const LzBlock* blocks, uint32_t nblocks, uint64_t total, uint16_t* blk,
                                                       uint64_t* keys) {
  lzh_keys_body(in_all, blocks, nblocks, total, blk, keys);
}
__global__ __launch_bounds__(256) void lzh_index_kernel(const uint64_t* keys, uint64_t nkeys, const LzBlock* blocks, uint32_t* idx) {
  lzh_index_body(keys, nkeys, blocks, idx);
}
__global__ __launch_bounds__(256) void lzh_search_kernel(const uint8_t* in_all, const uint64_t* keys, const uint32_t* idx, const uint16_t* blk,
                                                         const LzBlock* blocks, uint64_t total, uint4* res) {
  lzh_search_body(in_all, keys, idx, blk, blocks, total, res);
}

__global__ __launch_bounds__(256) void lzc_len_kernel(const LzBlock* blocks, uint32_t nblocks, uint64_t nslots, const LzTok* toks, const uint32_t* counts,
                                                      uint64_t* len, uint32_t* err) {
  lzc_len_body(blocks, nblocks, nslots, toks, counts, len, err);
}
__global__ __launch_bounds__(256) void lzc_sizes_kernel(const LzBlock* blocks, uint32_t nblocks, uint64_t nslots, const uint64_t* pos, uint32_t* sizes) {
  lzc_sizes_body(blocks, nblocks, nslots, pos, sizes);
}
__global__ __launch_bounds__(256) void lzc_match_kernel(const LzBlock* blocks, uint32_t nblocks, uint64_t nslots, const LzTok* toks, const uint32_t* counts,
                                                        const uint64_t* pos, const uint64_t* out_off, uint8_t* out) {
  lzc_match_body(blocks, nblocks, nslots, toks, counts, pos, out_off, out);
}
__global__ __launch_bounds__(256) void lzc_literal_kernel(const uint8_t* in_all, const LzBlock* blocks, uint32_t nblocks, uint64_t total, const LzTok* toks,
                                                          const uint32_t* counts, const uint64_t* pos, const uint64_t* out_off, uint8_t* out) {
  lzc_literal_body(in_all, blocks, nblocks, total, toks, counts, pos, out_off, out);
}

__global__ __launch_bounds__(64) void unlz_parse_kernel(const uint8_t* in_all, const UnlzStream* streams, uint4* toks, UnlzResult* res) {
  unlz_parse_body(in_all, streams, toks, res);
}
__global__ __launch_bounds__(64) void unlz_copy_kernel(const uint8_t* in_all, const UnlzStream* streams, const uint4* toks, const UnlzResult* res,
                                                       const uint64_t* out_off, uint8_t* out_all) {
  unlz_copy_body(in_all, streams, toks, res, out_off, out_all);
}

// device/lz77_decode_wide_kernel.h: a stream parsed in pieces, copied by pointer jumping
template <bool kBits>
__global__ __launch_bounds__(64) void unlzw_piece_kernel(const uint8_t* in_all, const UnlzWideStream* streams, const UnlzWideRef* refs, uint32_t piece,
                                                         uint4* prov, uint32_t* states, UnlzWidePieceOut* pieces) {
  unlzw_piece_body<kBits>(in_all, streams, refs, piece, prov, states, pieces);
}
template <bool kBits>
__global__ __launch_bounds__(64) void unlzw_stitch_kernel(const uint8_t* in_all, const UnlzWideStream* streams, uint32_t piece, const uint4* prov,
                                                          const uint32_t* states, const UnlzWidePieceOut* pieces, uint4* fin, UnlzWideAdopt* adopt,
                                                          UnlzWideOut* outs) {
  unlzw_stitch_body<kBits>(in_all, streams, piece, prov, states, pieces, fin, adopt, outs);
}
__global__ __launch_bounds__(256) void unlzw_finalize_kernel(const UnlzWideStream* streams, const UnlzWideRef* refs, uint32_t piece, const uint4* prov,
                                                             const UnlzWideAdopt* adopt, uint4* fin, UnlzWideOut* outs) {
  unlzw_finalize_body(streams, refs, piece, prov, adopt, fin, outs);
}
__global__ __launch_bounds__(256) void unlzw_link_kernel(const uint8_t* in_all, const UnlzWideStream* streams, const UnlzWidePlace* place, uint32_t nlive,
                                                         uint32_t total, const uint4* fin, uint32_t* w) {
  unlzw_link_body(in_all, streams, place, nlive, total, fin, w);
}
__global__ __launch_bounds__(256) void unlzw_jump_kernel(uint32_t* w, uint32_t total, uint32_t* flag) { unlzw_jump_body(w, total, flag); }
__global__ __launch_bounds__(256) void unlzw_emit_kernel(const uint32_t* w, uint32_t total, uint8_t* out) { unlzw_emit_body(w, total, out); }
__global__ __launch_bounds__(256) void unlzw_emit_placed_kernel(const uint32_t* w, const UnlzWidePlace* place, const uint64_t* dst_off, uint32_t nlive,
                                                                uint32_t total, uint8_t* out) {
  unlzw_emit_placed_body(w, place, dst_off, nlive, total, out);
}

__global__ __launch_bounds__(64) void unbwt_count_kernel(const uint8_t* in_all, const BwtStream* streams, uint32_t nstreams, uint32_t* hist) {
  unbwt_count_body(in_all, streams, nstreams, hist);
}
__global__ __launch_bounds__(256) void unbwt_scan_kernel(const BwtStream* streams, uint32_t* hist) { unbwt_scan_body(streams, hist); }
__global__ __launch_bounds__(64) void unbwt_link_kernel(const uint8_t* in_all, const BwtStream* streams, uint32_t nstreams, const uint32_t* hist,
                                                      uint32_t* link) {
  unbwt_link_body(in_all, streams, nstreams, hist, link);
}
__global__ __launch_bounds__(256) void unbwt_rank_kernel(const BwtStream* streams, uint32_t nstreams, uint32_t nsplit, const uint32_t* link, uint4* sp) {
  unbwt_rank_body(streams, nstreams, nsplit, link, sp);
}
__global__ __launch_bounds__(64) void unbwt_offsets_kernel(const BwtStream* streams, uint4* sp, uint32_t* status) { unbwt_offsets_body(streams, sp, status); }
__global__ __launch_bounds__(256) void unbwt_emit_kernel(const BwtStream* streams, uint32_t nstreams, uint32_t nsplit, const uint32_t* link, const uint4* sp,
                                                         const uint32_t* status, uint8_t* out_all) {
  unbwt_emit_body(streams, nstreams, nsplit, link, sp, status, out_all);
}

// device/bwt_decode_wide_kernel.h: blocks of 16 MiB and more (the count is the small form's; link, rank and emit are its bodies over
// 8-byte words)
__global__ __launch_bounds__(1024) void unbwt_wide_scan_kernel(const BwtStream* streams, uint32_t* hist) { unbwt_wide_scan_body(streams, hist); }
__global__ __launch_bounds__(64) void unbwt_wide_link_kernel(const uint8_t* in_all, const BwtStream* streams, uint32_t nstreams, const uint32_t* hist,
                                                             uint64_t* link) {
  unbwt_link_body(in_all, streams, nstreams, hist, link);
}
__global__ __launch_bounds__(256) void unbwt_wide_rank_kernel(const BwtStream* streams, uint32_t nstreams, uint32_t nsplit, const uint64_t* link, uint4* sp) {
  unbwt_rank_body(streams, nstreams, nsplit, link, sp);
}
__global__ __launch_bounds__(256) void unbwt_wide_rank2_kernel(const BwtStream* streams, const uint32_t* sp2_off, uint32_t nstreams, uint32_t nsplit2,
                                                               const uint4* sp, uint4* sp2) {
  unbwt_wide_rank2_body(streams, sp2_off, nstreams, nsplit2, sp, sp2);
}
__global__ __launch_bounds__(64) void unbwt_wide_offsets2_kernel(const BwtStream* streams, const uint32_t* sp2_off, uint4* sp2, uint32_t* status) {
  unbwt_wide_offsets2_body(streams, sp2_off, sp2, status);
}
__global__ __launch_bounds__(256) void unbwt_wide_offsets1_kernel(const BwtStream* streams, const uint32_t* sp2_off, uint32_t nstreams, uint32_t nsplit2,
                                                                  uint4* sp, const uint4* sp2, const uint32_t* status) {
  unbwt_wide_offsets1_body(streams, sp2_off, nstreams, nsplit2, sp, sp2, status);
}
__global__ __launch_bounds__(256) void unbwt_wide_emit_kernel(const BwtStream* streams, uint32_t nstreams, uint32_t nsplit, const uint64_t* link,
                                                              const uint4* sp, const uint32_t* status, uint8_t* out_all) {
  unbwt_emit_body(streams, nstreams, nsplit, link, sp, status, out_all);
}

__global__ __launch_bounds__(256) void une8_mark_kernel(const uint8_t* buf, const E8Block* blocks, uint32_t nblocks, uint32_t ntiles, uint32_t* cnt,
                                                        uint32_t* status) {
  une8_mark_body(buf, blocks, nblocks, ntiles, cnt, status);
}
__global__ __launch_bounds__(256) void une8_scatter_kernel(const uint8_t* buf, const E8Block* blocks, uint32_t nblocks, uint32_t ntiles,
                                                           const uint32_t* scan, uint32_t* list) {
  une8_scatter_body(buf, blocks, nblocks, ntiles, scan, list);
}
__global__ __launch_bounds__(256) void une8_walk_kernel(uint8_t* buf, const E8Block* blocks, uint32_t nblocks, uint32_t ntiles, const uint32_t* scan,
                                                        const uint32_t* list, uint32_t nseeds, uint32_t max_steps, uint32_t* status) {
  une8_walk_body(buf, blocks, nblocks, ntiles, scan, list, nseeds, max_steps, status);
}
__global__ __launch_bounds__(256) void e8f_mark_kernel(const uint8_t* buf, const E8Block* blocks, uint32_t nblocks, uint32_t ntiles, uint32_t* cnt,
                                                      uint32_t* status) {
  e8f_mark_body(buf, blocks, nblocks, ntiles, cnt, status);
}
__global__ __launch_bounds__(256) void e8f_scatter_kernel(const uint8_t* buf, const E8Block* blocks, uint32_t nblocks, uint32_t ntiles,
                                                         const uint32_t* scan, uint32_t* list) {
  e8f_scatter_body(buf, blocks, nblocks, ntiles, scan, list);
}
__global__ __launch_bounds__(256) void e8f_walk_kernel(uint8_t* buf, const E8Block* blocks, uint32_t nblocks, uint32_t ntiles, const uint32_t* scan,
                                                      const uint32_t* list, uint32_t nseeds, uint32_t max_steps, uint32_t* status) {
  e8f_walk_body(buf, blocks, nblocks, ntiles, scan, list, nseeds, max_steps, status);
}

__global__ __launch_bounds__(64) void frag_walk_kernel(const uint8_t* buf, const FragJob* jobs, uint32_t njobs, FragParams P, FragRec* recs,
                                                       FragResult* res) {
  frag_walk_body(buf, jobs, njobs, P, recs, res);
}

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

size_t sa_workspace_bytes(uint64_t total, uint32_t nblocks) {
  size_t sort_tmp = 0, scan_tmp = 0;
  (void)rocprim::radix_sort_pairs(nullptr, sort_tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)total, 0, 64);
  (void)rocprim::inclusive_scan(nullptr, scan_tmp, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)total, rocprim::plus<uint32_t>());
  const size_t a = (size_t)((total + 63) & ~63ull);
  // keys x 2, vals x 2, rank, flags / scan, blk, off, pointers, library scratch
  return a * (8 + 8 + 4 + 4 + 4 + 4 + 2) + ((size_t)nblocks + 2) * 16 + (sort_tmp > scan_tmp ? sort_tmp : scan_tmp) + 4096;
}

// d_in[b] -> bytes of block b ON THE DEVICE, d_off[0..nblocks] = exclusive prefix sums of the lengths (device), total = d_off[nblocks];
// d_sa receives the suffix arrays back to back (d_sa + off[b] = block b's).  `ws` = sa_workspace_bytes(total, nblocks) bytes of device memory.
hipError_t build_suffix_arrays(const uint8_t* const* d_in, const uint64_t* d_off, uint32_t nblocks, uint64_t total, uint32_t max_len,
                               uint32_t* d_sa, void* ws, size_t ws_bytes, hipStream_t st, uint32_t* rounds_out, SaSideArrays* side) {
  if (!total) return hipSuccess;
  if (nblocks > 65535u || max_len >= (1u << 24) || total >= (1ull << 32)) return hipErrorInvalidValue;
  const size_t a = (size_t)((total + 63) & ~63ull);
  uint8_t* p = (uint8_t*)ws;
  uint64_t* keys = (uint64_t*)p; p += a * 8;
  uint64_t* keys2 = (uint64_t*)p; p += a * 8;
  uint32_t* vals = (uint32_t*)p; p += a * 4;
  uint32_t* vals2 = (uint32_t*)p; p += a * 4;
  uint32_t* rank = (uint32_t*)p; p += a * 4;
  uint32_t* flags = (uint32_t*)p; p += a * 4;
  uint16_t* blk = (uint16_t*)p; p += a * 2;
  p = (uint8_t*)(((uintptr_t)p + 255) & ~(uintptr_t)255);
  void* tmp = p;
  const size_t tmp_bytes = ws_bytes - (size_t)(p - (uint8_t*)ws);
  const unsigned g = grid_for(total);
  hipLaunchKernelGGL(sa_init_kernel, dim3(g), dim3(256), 0, st, d_in, d_off, nblocks, total, rank, blk);
  const unsigned key_bits = sa_key_bits(nblocks);
  uint32_t h = 1, rounds = 0;
  for (;; h <<= 1) {
    hipLaunchKernelGGL(sa_keys_kernel, dim3(g), dim3(256), 0, st, rank, blk, d_off, total, h, keys, vals);
    size_t need = tmp_bytes;
    hipError_t e = rocprim::radix_sort_pairs(tmp, need, keys, keys2, vals, vals2, (size_t)total, 0, key_bits, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sa_flags_kernel, dim3(g), dim3(256), 0, st, keys2, total, flags);
    need = tmp_bytes;
    e = rocprim::inclusive_scan(tmp, need, flags, flags, (size_t)total, rocprim::plus<uint32_t>(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sa_rename_kernel, dim3(g), dim3(256), 0, st, keys2, vals2, flags, d_off, total, rank);
    ++rounds;
    uint32_t names = 0;                                              // the last prefix sum
    e = hipMemcpyAsync(&names, flags + (total - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return e;
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) return e;
    if (sa_round_is_last(names, total, h, max_len)) break;
  }
  hipLaunchKernelGGL(sa_invert_kernel, dim3(g), dim3(256), 0, st, rank, blk, d_off, total, d_sa);
  if (rounds_out) *rounds_out = rounds;
  if (side) { side->rank = rank; side->blk = blk; }
  return hipGetLastError();
}

// The wide sorter (device/sa_wide_kernel.h): one block of 1 <= n < 2^31 bytes.  Keys x 2, values x 2 (the sort's double
// buffers: the library ping-pongs between them and needs no copies of its own), rank, flags / scan -- 32 bytes per element --
// and the library's scratch.  No element-to-block map.
size_t sa_wide_workspace_bytes(uint64_t n) {
  size_t sort_tmp = 0, scan_tmp = 0;
  rocprim::double_buffer<uint64_t> k((uint64_t*)nullptr, (uint64_t*)nullptr);
  rocprim::double_buffer<uint32_t> v((uint32_t*)nullptr, (uint32_t*)nullptr);
  (void)rocprim::radix_sort_pairs(nullptr, sort_tmp, k, v, (size_t)n, 0, 64);
  (void)rocprim::inclusive_scan(nullptr, scan_tmp, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, rocprim::plus<uint32_t>());
  const size_t a = (size_t)((n + 63) & ~63ull);
  return a * (8 + 8 + 4 + 4 + 4 + 4) + (sort_tmp > scan_tmp ? sort_tmp : scan_tmp) + 4096;
}

// d_in: the block on the device.  d_sa (may be null: the ranks are all the caller wants) receives the array.  *rank_out: the
// final ranks in the workspace (rank[i] - 1 = position of suffix i in the array), valid until the workspace is used again.
// rank_bits: 0 = sa_wide_rank_bits(n); a test forces a wider field.  Synchronises `st` once per round.
hipError_t build_suffix_array_wide(const uint8_t* d_in, uint32_t n, uint32_t* d_sa, void* ws, size_t ws_bytes, hipStream_t st, uint32_t* rounds_out,
                                   const uint32_t** rank_out, unsigned rank_bits) {
  if (rounds_out) *rounds_out = 0;
  if (!n) return hipSuccess;
  const unsigned r = rank_bits ? rank_bits : sa_wide_rank_bits(n);
  if (n >= (1u << 31) || r > 32 || r < sa_wide_rank_bits(n) || ws_bytes < sa_wide_workspace_bytes(n)) return hipErrorInvalidValue;
  const size_t a = (size_t)(((uint64_t)n + 63) & ~63ull);
  uint8_t* p = (uint8_t*)ws;
  uint64_t* keys = (uint64_t*)p; p += a * 8;
  uint64_t* keys2 = (uint64_t*)p; p += a * 8;
  uint32_t* vals = (uint32_t*)p; p += a * 4;
  uint32_t* vals2 = (uint32_t*)p; p += a * 4;
  uint32_t* rank = (uint32_t*)p; p += a * 4;
  uint32_t* flags = (uint32_t*)p; p += a * 4;
  p = (uint8_t*)(((uintptr_t)p + 255) & ~(uintptr_t)255);
  void* tmp = p;
  const size_t tmp_bytes = ws_bytes - (size_t)(p - (uint8_t*)ws);
  const unsigned g = grid_for(n);
  hipLaunchKernelGGL(sa_wide_init_kernel, dim3(g), dim3(256), 0, st, d_in, n, rank);
  uint32_t h = 1, rounds = 0;
  for (;; h <<= 1) {
    const unsigned w = sa_wide_field_bits(r, h);
    hipLaunchKernelGGL(sa_wide_keys_kernel, dim3(g), dim3(256), 0, st, (const uint32_t*)rank, n, h, (uint32_t)w, keys, vals);
    rocprim::double_buffer<uint64_t> kb(keys, keys2);
    rocprim::double_buffer<uint32_t> vb(vals, vals2);
    size_t need = tmp_bytes;
    hipError_t e = rocprim::radix_sort_pairs(tmp, need, kb, vb, (size_t)n, 0, 2 * w, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sa_flags_kernel, dim3(g), dim3(256), 0, st, (const uint64_t*)kb.current(), (uint64_t)n, flags);
    need = tmp_bytes;
    e = rocprim::inclusive_scan(tmp, need, flags, flags, (size_t)n, rocprim::plus<uint32_t>(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sa_wide_rename_kernel, dim3(g), dim3(256), 0, st, (const uint32_t*)vb.current(), (const uint32_t*)flags, n, rank);
    ++rounds;
    uint32_t names = 0;                                              // the last prefix sum
    e = hipMemcpyAsync(&names, flags + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return e;
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) return e;
    if (sa_round_is_last(names, n, h, n)) break;
  }
  if (d_sa) hipLaunchKernelGGL(sa_wide_invert_kernel, dim3(g), dim3(256), 0, st, (const uint32_t*)rank, n, d_sa);
  if (rounds_out) *rounds_out = rounds;
  if (rank_out) *rank_out = rank;
  return hipGetLastError();
}

// the BWT's last column of the block build_suffix_array_wide has just ranked: n + 1 bytes at d_out, the index at d_idx[0]
hipError_t launch_bwt_wide(const uint8_t* d_in, const uint32_t* d_rank, uint32_t n, uint8_t* d_out, uint32_t* d_idx, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(bwt_wide_kernel, dim3(grid_for(n)), dim3(256), 0, st, d_in, d_rank, n, d_out, d_idx);
  return hipGetLastError();
}

hipError_t launch_sort_preprocessors(const uint8_t* in_all, const uint32_t* sa_all, const SaSideArrays& side, const LzBlock* blocks, uint32_t nblocks,
                                     uint64_t total, bool any_lz, bool any_bwt, void* res, LzTok* toks, uint32_t* counts, uint8_t* bwt_out,
                                     uint32_t* bwt_idx, hipStream_t st, const LzCodes* codes) {
  if (!total || !nblocks) return hipSuccess;
  const unsigned g = grid_for(total);
  if (any_lz) {
    hipLaunchKernelGGL(lz77_search_kernel, dim3(g), dim3(256), 0, st, in_all, sa_all, (const uint32_t*)side.rank, (const uint16_t*)side.blk, blocks, total, (uint4*)res);
    hipLaunchKernelGGL(lz77_walk_kernel, dim3(nblocks), dim3(64), 0, st, blocks, (const uint4*)res, toks, counts);
    if (codes) {
      const hipError_t e = launch_lz77_code_lengths(blocks, nblocks, toks, counts, *codes, st);
      if (e != hipSuccess) return e;
    }
  }
  if (any_bwt)
    hipLaunchKernelGGL(bwt_emit_kernel, dim3(g), dim3(256), 0, st, in_all, sa_all, (const uint16_t*)side.blk, blocks, total, bwt_out, bwt_idx);
  return hipGetLastError();
}

// device/lz77_wide_kernel.h behind build_suffix_array_wide: search, piece walk, stitch, gather.  blocks: the one-entry table (off 0,
// tok_off 0, tok_cap slots at toks); W.n = blocks[0].n, W.npieces pieces of W.piece positions with W.slot_cap slots each at prov.
hipError_t launch_lz77_wide(const uint8_t* d_in, const uint32_t* d_sa, const uint32_t* d_rank, const LzBlock* blocks, LzWideParams W, uint32_t tok_cap,
                            void* res, LzTok* prov, LzWidePiece* pieces, LzWideAdopt* adopt, LzTok* toks, LzWideResult* out, hipStream_t st) {
  if (!W.n) return hipSuccess;
  if (W.n >= (1u << 31) || W.piece < 64u || W.piece % 64u || W.npieces != (uint32_t)(((uint64_t)W.n + W.piece - 1u) / W.piece) || !W.slot_cap)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(lz77_wide_search_kernel, dim3(grid_for(W.n)), dim3(256), 0, st, d_in, d_sa, d_rank, blocks, (uint4*)res);
  hipLaunchKernelGGL(lz77_wide_walk_kernel, dim3(W.npieces), dim3(64), 0, st, W, (const uint4*)res, prov, pieces);
  hipLaunchKernelGGL(lz77_wide_stitch_kernel, dim3(1), dim3(64), 0, st, W, (const uint4*)res, (const LzTok*)prov, (const LzWidePiece*)pieces, toks, tok_cap,
                     adopt, out);
  hipLaunchKernelGGL(lz77_wide_gather_kernel, dim3(W.npieces), dim3(256), 0, st, W, (const LzTok*)prov, (const LzWideAdopt*)adopt, toks, tok_cap);
  return hipGetLastError();
}

size_t lzh_workspace_bytes(uint64_t total, uint64_t nkeys, uint64_t nidx) {
  size_t sort_tmp = 0;
  if (nkeys) (void)rocprim::radix_sort_keys(nullptr, sort_tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)nkeys, 0, 64);
  // keys x 2, the element -> block map, the index, library scratch
  return 2 * up256((size_t)nkeys * 8) + up256((size_t)total * 2) + up256((size_t)nidx * 4) + up256(sort_tmp) + 4096;
}

// The LZ77 parse through the hash table for a whole batch (device/lz77_hash_kernel.h): blocks[b] with ht_bits != 0, key_off /
// idx_off / nkeys / ins_end / idx_bits filled in by the caller (nkeys, nidx: the sums over the batch).
hipError_t launch_hash_parse(const uint8_t* in_all, const LzBlock* blocks, uint32_t nblocks, uint64_t total, uint64_t nkeys, uint64_t nidx, void* ws,
                             size_t ws_bytes, void* res, LzTok* toks, uint32_t* counts, hipStream_t st, const LzCodes* codes) {
  if (!total || !nblocks) return hipSuccess;
  if (nblocks > 65535u || total >= (1ull << 32) || ws_bytes < lzh_workspace_bytes(total, nkeys, nidx)) return hipErrorInvalidValue;
  uint8_t* p = (uint8_t*)ws;
  uint64_t* keys = (uint64_t*)p; p += up256((size_t)nkeys * 8);
  uint64_t* keys2 = (uint64_t*)p; p += up256((size_t)nkeys * 8);
  uint16_t* blk = (uint16_t*)p; p += up256((size_t)total * 2);
  uint32_t* idx = (uint32_t*)p; p += up256((size_t)nidx * 4);
  void* tmp = p;
  const size_t tmp_bytes = ws_bytes - (size_t)(p - (uint8_t*)ws);
  hipLaunchKernelGGL(lzh_keys_kernel, dim3(grid_for(total)), dim3(256), 0, st, in_all, blocks, nblocks, total, blk, keys);
  if (nkeys) {
    unsigned blk_bits = 1;
    while ((1u << blk_bits) < nblocks) ++blk_bits;
    size_t need = tmp_bytes;
    const hipError_t e = rocprim::radix_sort_keys(tmp, need, keys, keys2, (size_t)nkeys, 0, 48 + blk_bits, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzh_index_kernel, dim3(grid_for(nkeys)), dim3(256), 0, st, (const uint64_t*)keys2, nkeys, blocks, idx);
  }
  hipLaunchKernelGGL(lzh_search_kernel, dim3(grid_for(total)), dim3(256), 0, st, in_all, (const uint64_t*)keys2, (const uint32_t*)idx,
                     (const uint16_t*)blk, blocks, total, (uint4*)res);
  hipLaunchKernelGGL(lz77_walk_kernel, dim3(nblocks), dim3(64), 0, st, blocks, (const uint4*)res, toks, counts);
  if (codes) {
    const hipError_t e = launch_lz77_code_lengths(blocks, nblocks, toks, counts, *codes, st);
    if (e != hipSuccess) return e;
  }
  return hipGetLastError();
}

size_t lzc_scan_bytes(uint64_t nslots) {
  size_t scan_tmp = 0;
  (void)rocprim::exclusive_scan(nullptr, scan_tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)(nslots + 1), rocprim::plus<uint64_t>());
  return up256(scan_tmp) + 256;
}

// Stages (a) and (b) of device/lz77_codes_kernel.h: lengths, the scan (64-bit: 2 GiB of input is more than 2^32 bits), sizes.
hipError_t launch_lz77_code_lengths(const LzBlock* blocks, uint32_t nblocks, const LzTok* toks, const uint32_t* counts, const LzCodes& c, hipStream_t st) {
  if (!nblocks) return hipSuccess;
  if (!c.pos || !c.sizes || !c.tmp || c.nslots < nblocks || c.nslots >= (1ull << 32) || c.tmp_bytes < lzc_scan_bytes(c.nslots)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lzc_len_kernel, dim3(grid_for(c.nslots + 1)), dim3(256), 0, st, blocks, nblocks, c.nslots, toks, counts, c.pos, c.sizes + nblocks);
  size_t need = c.tmp_bytes;
  const hipError_t e = rocprim::exclusive_scan(c.tmp, need, c.pos, c.pos, (uint64_t)0, (size_t)(c.nslots + 1), rocprim::plus<uint64_t>(), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(lzc_sizes_kernel, dim3(grid_for(nblocks)), dim3(256), 0, st, blocks, nblocks, c.nslots, (const uint64_t*)c.pos, c.sizes);
  return hipGetLastError();
}

// Stage (d): `out` is zeroed (level 1 only ever ORs into it), the streams lie where out_off says.
hipError_t launch_lz77_emit(const uint8_t* in_all, const LzBlock* blocks, uint32_t nblocks, uint64_t total, const LzTok* toks, const uint32_t* counts,
                            const LzCodes& c, const uint64_t* out_off, uint8_t* out, hipStream_t st) {
  if (!nblocks) return hipSuccess;
  hipLaunchKernelGGL(lzc_match_kernel, dim3(grid_for(c.nslots)), dim3(256), 0, st, blocks, nblocks, c.nslots, toks, counts, (const uint64_t*)c.pos, out_off, out);
  if (total)
    hipLaunchKernelGGL(lzc_literal_kernel, dim3(grid_for(total)), dim3(256), 0, st, in_all, blocks, nblocks, total, toks, counts, (const uint64_t*)c.pos,
                       out_off, out);
  return hipGetLastError();
}

// device/lz77_decode_kernel.h, stage (a): the streams' tokens and {out_len, ntok, status} per stream
hipError_t launch_unlz_parse(const uint8_t* in_all, const UnlzStream* streams, uint32_t nstreams, void* toks, UnlzResult* res, hipStream_t st) {
  if (!nstreams) return hipSuccess;
  if (nstreams > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(unlz_parse_kernel, dim3(nstreams), dim3(64), 0, st, in_all, streams, (uint4*)toks, res);
  return hipGetLastError();
}

// stage (c): the outputs, stream b's at out_all + out_off[b]
hipError_t launch_unlz_copy(const uint8_t* in_all, const UnlzStream* streams, uint32_t nstreams, const void* toks, const UnlzResult* res,
                            const uint64_t* out_off, uint8_t* out_all, hipStream_t st) {
  if (!nstreams) return hipSuccess;
  if (nstreams > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(unlz_copy_kernel, dim3(nstreams), dim3(64), 0, st, in_all, streams, (const uint4*)toks, res, out_off, out_all);
  return hipGetLastError();
}

// device/lz77_decode_wide_kernel.h, the first half: the pieces' lists, the stitch (over `adopt`, zeroed here), the final lists.
// Leaves outs[b] = {{out_len, ntok, status}, the first failing token's key (all ones: none), the counts}.
// level: the batch's (1 or 2; a stream of the other is declined).
hipError_t launch_unlz_wide_parse(uint32_t level, const uint8_t* in_all, const UnlzWideStream* streams, uint32_t nstreams, const UnlzWideRef* refs, uint32_t npieces,
                                  uint32_t piece, void* prov, uint32_t* states, UnlzWidePieceOut* pieces, void* fin, UnlzWideAdopt* adopt, UnlzWideOut* outs,
                                  hipStream_t st) {
  if (!nstreams) return hipSuccess;
  const uint64_t fblocks = (uint64_t)npieces * ((piece + 255u) / 256u);
  if (fblocks >= (1ull << 31)) return hipErrorInvalidValue;
  if (npieces) {
    hipError_t rc = hipMemsetAsync(adopt, 0, sizeof(UnlzWideAdopt) * (size_t)npieces, st);
    if (rc != hipSuccess) return rc;
    if (level == 1u) hipLaunchKernelGGL(unlzw_piece_kernel<true>, dim3(npieces), dim3(64), 0, st, in_all, streams, refs, piece, (uint4*)prov, states, pieces);
    else hipLaunchKernelGGL(unlzw_piece_kernel<false>, dim3(npieces), dim3(64), 0, st, in_all, streams, refs, piece, (uint4*)prov, states, pieces);
  }
  if (level == 1u)
    hipLaunchKernelGGL(unlzw_stitch_kernel<true>, dim3(nstreams), dim3(64), 0, st, in_all, streams, piece, (const uint4*)prov, (const uint32_t*)states,
                       (const UnlzWidePieceOut*)pieces, (uint4*)fin, adopt, outs);
  else
    hipLaunchKernelGGL(unlzw_stitch_kernel<false>, dim3(nstreams), dim3(64), 0, st, in_all, streams, piece, (const uint4*)prov, (const uint32_t*)states,
                       (const UnlzWidePieceOut*)pieces, (uint4*)fin, adopt, outs);
  if (npieces)
    hipLaunchKernelGGL(unlzw_finalize_kernel, dim3((unsigned)fblocks), dim3(256), 0, st, streams, refs, piece, (const uint4*)prov,
                       (const UnlzWideAdopt*)adopt, (uint4*)fin, outs);
  return hipGetLastError();
}
// ... the second half: every output byte's word, from the final lists of the `nlive` decoded streams (`total` bytes in all)
hipError_t launch_unlz_wide_link(const uint8_t* in_all, const UnlzWideStream* streams, const UnlzWidePlace* place, uint32_t nlive, uint32_t total,
                                 const void* fin, uint32_t* w, hipStream_t st) {
  if (!total) return hipSuccess;
  hipLaunchKernelGGL(unlzw_link_kernel, dim3(grid_for(total)), dim3(256), 0, st, in_all, streams, place, nlive, total, (const uint4*)fin, w);
  return hipGetLastError();
}
// ... one jump round; *flag (zero before) becomes 1 if another is needed
hipError_t launch_unlz_wide_jump(uint32_t* w, uint32_t total, uint32_t* flag, hipStream_t st) {
  if (!total) return hipSuccess;
  hipLaunchKernelGGL(unlzw_jump_kernel, dim3(grid_for(total)), dim3(256), 0, st, w, total, flag);
  return hipGetLastError();
}
// ... and the bytes
hipError_t launch_unlz_wide_emit(const uint32_t* w, uint32_t total, uint8_t* out, hipStream_t st) {
  if (!total) return hipSuccess;
  hipLaunchKernelGGL(unlzw_emit_kernel, dim3(grid_for(total)), dim3(256), 0, st, w, total, out);
  return hipGetLastError();
}
// ... or the bytes of stream place[a] at out + dst_off[a], for the filter behind the stage (the words stay packed)
hipError_t launch_unlz_wide_emit_placed(const uint32_t* w, const UnlzWidePlace* place, const uint64_t* dst_off, uint32_t nlive, uint32_t total, uint8_t* out,
                                        hipStream_t st) {
  if (!total) return hipSuccess;
  if (!nlive) return hipErrorInvalidValue;
  hipLaunchKernelGGL(unlzw_emit_placed_kernel, dim3(grid_for(total)), dim3(256), 0, st, w, place, dst_off, nlive, total, out);
  return hipGetLastError();
}

// device/bwt_decode_kernel.h: the six stages for a batch of admitted streams, one after the other on `st`
hipError_t launch_bwt_decode(const uint8_t* in_all, const BwtStream* streams, uint32_t nstreams, uint32_t ntiles, uint32_t nsplit, uint32_t* hist,
                             uint32_t* link, void* splitters, uint32_t* status, uint8_t* out_all, hipStream_t st) {
  if (!nstreams) return hipSuccess;
  if (nstreams > 65535u || !ntiles || !nsplit) return hipErrorInvalidValue;
  uint4* sp = (uint4*)splitters;
  const uint32_t spb = (nsplit + 255u) / 256u;
  hipLaunchKernelGGL(unbwt_count_kernel, dim3(ntiles), dim3(64), 0, st, in_all, streams, nstreams, hist);
  hipLaunchKernelGGL(unbwt_scan_kernel, dim3(nstreams), dim3(256), 0, st, streams, hist);
  hipLaunchKernelGGL(unbwt_link_kernel, dim3(ntiles), dim3(64), 0, st, in_all, streams, nstreams, (const uint32_t*)hist, link);
  hipLaunchKernelGGL(unbwt_rank_kernel, dim3(spb), dim3(256), 0, st, streams, nstreams, nsplit, (const uint32_t*)link, sp);
  hipLaunchKernelGGL(unbwt_offsets_kernel, dim3(nstreams), dim3(64), 0, st, streams, sp, status);
  hipLaunchKernelGGL(unbwt_emit_kernel, dim3(spb), dim3(256), 0, st, streams, nstreams, nsplit, (const uint32_t*)link, (const uint4*)sp,
                     (const uint32_t*)status, out_all);
  return hipGetLastError();
}

// device/bwt_decode_wide_kernel.h: the eight stages for a batch of admitted wide streams, one after the other on `st`
hipError_t launch_bwt_decode_wide(const uint8_t* in_all, const BwtStream* streams, const uint32_t* sp2_off, uint32_t nstreams, uint32_t ntiles,
                                  uint32_t nsplit, uint32_t nsplit2, uint32_t* hist, uint64_t* link, void* splitters, void* splitters2, uint32_t* status,
                                  uint8_t* out_all, hipStream_t st) {
  if (!nstreams) return hipSuccess;
  if (nstreams > 65535u || !ntiles || !nsplit || !nsplit2) return hipErrorInvalidValue;
  uint4* sp = (uint4*)splitters;
  uint4* sp2 = (uint4*)splitters2;
  const uint32_t spb = (nsplit + 255u) / 256u, spb2 = (nsplit2 + 255u) / 256u;
  hipLaunchKernelGGL(unbwt_count_kernel, dim3(ntiles), dim3(64), 0, st, in_all, streams, nstreams, hist);
  hipLaunchKernelGGL(unbwt_wide_scan_kernel, dim3(nstreams), dim3(256 * kBwtScanParts), 0, st, streams, hist);
  hipLaunchKernelGGL(unbwt_wide_link_kernel, dim3(ntiles), dim3(64), 0, st, in_all, streams, nstreams, (const uint32_t*)hist, link);
  hipLaunchKernelGGL(unbwt_wide_rank_kernel, dim3(spb), dim3(256), 0, st, streams, nstreams, nsplit, (const uint64_t*)link, sp);
  hipLaunchKernelGGL(unbwt_wide_rank2_kernel, dim3(spb2), dim3(256), 0, st, streams, sp2_off, nstreams, nsplit2, (const uint4*)sp, sp2);
  hipLaunchKernelGGL(unbwt_wide_offsets2_kernel, dim3(nstreams), dim3(64), 0, st, streams, sp2_off, sp2, status);
  hipLaunchKernelGGL(unbwt_wide_offsets1_kernel, dim3(spb2), dim3(256), 0, st, streams, sp2_off, nstreams, nsplit2, sp, (const uint4*)sp2,
                     (const uint32_t*)status);
  hipLaunchKernelGGL(unbwt_wide_emit_kernel, dim3(spb), dim3(256), 0, st, streams, nstreams, nsplit, (const uint64_t*)link, (const uint4*)sp,
                     (const uint32_t*)status, out_all);
  return hipGetLastError();
}

size_t une8_scan_bytes(uint32_t ntiles) {
  size_t scan_tmp = 0;
  (void)rocprim::exclusive_scan(nullptr, scan_tmp, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)2 * ntiles + 1, rocprim::plus<uint32_t>());
  return up256(scan_tmp) + 256;
}

// device/e8e9_kernel.h, the first half: the counts per tile, scanned in place, and the blocks' statuses zeroed
hipError_t launch_une8_mark(const uint8_t* buf, const E8Block* blocks, uint32_t nblocks, uint32_t ntiles, uint32_t* cnt, uint32_t* status, void* tmp,
                            size_t tmp_bytes, hipStream_t st) {
  if (!nblocks) return hipSuccess;
  if (nblocks > 65535u || ntiles < nblocks || ntiles >= (1u << 30) || tmp_bytes < une8_scan_bytes(ntiles)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(une8_mark_kernel, dim3(ntiles), dim3(256), 0, st, buf, blocks, nblocks, ntiles, cnt, status);
  size_t need = tmp_bytes;
  const hipError_t e = rocprim::exclusive_scan(tmp, need, cnt, cnt, 0u, (size_t)2 * ntiles + 1, rocprim::plus<uint32_t>(), st);
  if (e != hipSuccess) return e;
  return hipGetLastError();
}

// ... the second half: the list (nlist = scan[2 * ntiles] words, the first nseeds = scan[ntiles] of them seeds), then the walk
hipError_t launch_une8_walk(uint8_t* buf, const E8Block* blocks, uint32_t nblocks, uint32_t ntiles, const uint32_t* scan, uint32_t* list,
                            uint32_t nseeds, uint32_t max_steps, uint32_t* status, hipStream_t st) {
  if (!nblocks || !nseeds) return hipSuccess;                   // (no seed: no hit, the breaks alone are not needed)
  if (nblocks > 65535u || ntiles < nblocks) return hipErrorInvalidValue;
  hipLaunchKernelGGL(une8_scatter_kernel, dim3(ntiles), dim3(256), 0, st, (const uint8_t*)buf, blocks, nblocks, ntiles, scan, list);
  hipLaunchKernelGGL(une8_walk_kernel, dim3(grid_for(nseeds)), dim3(256), 0, st, buf, blocks, nblocks, ntiles, scan, (const uint32_t*)list, nseeds,
                     max_steps, status);
  return hipGetLastError();
}

// device/e8e9_forward_kernel.h, the two halves as the inverse's: the same arguments, the same checks, the same scratch
hipError_t launch_e8f_mark(const uint8_t* buf, const E8Block* blocks, uint32_t nblocks, uint32_t ntiles, uint32_t* cnt, uint32_t* status, void* tmp,
                           size_t tmp_bytes, hipStream_t st) {
  if (!nblocks) return hipSuccess;
  if (nblocks > 65535u || ntiles < nblocks || ntiles >= (1u << 30) || tmp_bytes < une8_scan_bytes(ntiles)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(e8f_mark_kernel, dim3(ntiles), dim3(256), 0, st, buf, blocks, nblocks, ntiles, cnt, status);
  size_t need = tmp_bytes;
  const hipError_t e = rocprim::exclusive_scan(tmp, need, cnt, cnt, 0u, (size_t)2 * ntiles + 1, rocprim::plus<uint32_t>(), st);
  if (e != hipSuccess) return e;
  return hipGetLastError();
}

hipError_t launch_e8f_walk(uint8_t* buf, const E8Block* blocks, uint32_t nblocks, uint32_t ntiles, const uint32_t* scan, uint32_t* list,
                           uint32_t nseeds, uint32_t max_steps, uint32_t* status, hipStream_t st) {
  if (!nblocks || !nseeds) return hipSuccess;                   // (no seed: no hit, the breaks alone are not needed)
  if (nblocks > 65535u || ntiles < nblocks) return hipErrorInvalidValue;
  hipLaunchKernelGGL(e8f_scatter_kernel, dim3(ntiles), dim3(256), 0, st, (const uint8_t*)buf, blocks, nblocks, ntiles, scan, list);
  hipLaunchKernelGGL(e8f_walk_kernel, dim3(grid_for(nseeds)), dim3(256), 0, st, buf, blocks, nblocks, ntiles, scan, (const uint32_t*)list, nseeds,
                     max_steps, status);
  return hipGetLastError();
}

// device/fragment_kernel.h: a wavefront per job
hipError_t launch_frag_walk(const uint8_t* buf, const FragJob* jobs, uint32_t njobs, FragParams P, FragRec* recs, FragResult* res, hipStream_t st) {
  if (!njobs) return hipSuccess;
  if (!P.min_frag || P.max_frag < P.min_frag) return hipErrorInvalidValue;
  hipLaunchKernelGGL(frag_walk_kernel, dim3(njobs), dim3(64), 0, st, buf, jobs, njobs, P, recs, res);
  return hipGetLastError();
}

}  // namespace zpq
