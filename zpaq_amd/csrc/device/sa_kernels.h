// Launch prototypes of device/sa_kernels.hip: suffix arrays of many blocks at once (prefix doubling, rocPRIM sorts).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "layout.h"
#include "lz77_wide_layout.h"

namespace zpq {
// what the sorter leaves in its workspace besides the arrays: rank[i] - 1 = position of suffix i in its block's suffix array (the
// inverse array), blk[i] = block of element i
struct SaSideArrays { uint32_t* rank = nullptr; uint16_t* blk = nullptr; };
// device memory build_suffix_arrays needs for `total` bytes of input in `nblocks` blocks
size_t sa_workspace_bytes(uint64_t total, uint32_t nblocks);
// what the stages behind the walk that write LZBuffer's codes need (described with launch_lz77_code_lengths below)
struct LzCodes { uint64_t nslots = 0; uint64_t* pos = nullptr; void* tmp = nullptr; size_t tmp_bytes = 0; uint32_t* sizes = nullptr; };
// d_in[b] -> block b's bytes on the device; d_off[0..nblocks] = exclusive prefix sums of the lengths; d_sa: the arrays back
// to back (block b's at d_sa + off[b]); max_len < 2^24, nblocks < 65536, total < 2^32.  Synchronises `st` once per round.
hipError_t build_suffix_arrays(const uint8_t* const* d_in, const uint64_t* d_off, uint32_t nblocks, uint64_t total, uint32_t max_len,
                               uint32_t* d_sa, void* ws, size_t ws_bytes, hipStream_t st, uint32_t* rounds_out, SaSideArrays* side = nullptr);
// The wide sorter (device/sa_wide_kernel.h): ONE block of 1 <= n < 2^31 bytes at d_in, the key two rank fields of
// sa_wide_rank_bits(n) bits (rank_bits != 0 forces a wider field: tests).  ws: sa_wide_workspace_bytes(n) bytes -- 32 per element
// and the library's scratch.  d_sa receives the array, or is null when the caller goes on from the ranks: *rank_out points at
// them in the workspace (rank[i] - 1 = position of suffix i in the array).  Synchronises `st` once per round.
size_t sa_wide_workspace_bytes(uint64_t n);
hipError_t build_suffix_array_wide(const uint8_t* d_in, uint32_t n, uint32_t* d_sa, void* ws, size_t ws_bytes, hipStream_t st, uint32_t* rounds_out,
                                   const uint32_t** rank_out = nullptr, unsigned rank_bits = 0);
// ... and the BWT's last column from those ranks, in preprocess_block's layout: n + 1 bytes at d_out, the index of the whole
// string at d_idx[0]
hipError_t launch_bwt_wide(const uint8_t* d_in, const uint32_t* d_rank, uint32_t n, uint8_t* d_out, uint32_t* d_idx, hipStream_t st);
// Behind the sort, for the same batch (device/lz77_kernel.h): the LZ77 parse of the blocks of kind 1 / 2 -- 16 bytes of decisions
// per element in `res`, then the matches taken in toks[blocks[b].tok_off ..) and their number in counts[b] -- and the BWT of
// the blocks of kind 3 (n + 1 bytes at bwt_out + off + b, the index of the whole string in bwt_idx[b]).  in_all: the blocks'
// bytes back to back like the arrays.
hipError_t launch_sort_preprocessors(const uint8_t* in_all, const uint32_t* sa_all, const SaSideArrays& side, const LzBlock* blocks, uint32_t nblocks,
                                     uint64_t total, bool any_lz, bool any_bwt, void* res, LzTok* toks, uint32_t* counts, uint8_t* bwt_out,
                                     uint32_t* bwt_idx, hipStream_t st, const LzCodes* codes = nullptr);
// The LZ77 parse of the ONE block build_suffix_array_wide has just sorted (device/lz77_wide_kernel.h): the search (16 bytes of
// decisions per position in `res`), the walk of W.npieces pieces of W.piece positions from provisional starts (W.slot_cap token
// slots each in `prov`, {count, exit state} in `pieces`), the stitch (one wavefront: what it adopts of each piece in `adopt`, its
// own tokens in `toks`, the counts in `out`) and the gather of the adopted tokens into toks[0 .. tok_cap).  blocks: the one-entry
// table with the search parameters.  out->count is the list's length (more than tok_cap: incomplete) -- the coder's counts[0].
hipError_t launch_lz77_wide(const uint8_t* d_in, const uint32_t* d_sa, const uint32_t* d_rank, const LzBlock* blocks, LzWideParams W, uint32_t tok_cap,
                            void* res, LzTok* prov, LzWidePiece* pieces, LzWideAdopt* adopt, LzTok* toks, LzWideResult* out, hipStream_t st);
// The LZ77 parse through LZBuffer's hash table for a batch (device/lz77_hash_kernel.h): keys, one radix sort, the index of slot
// prefixes, the search (16 bytes of decisions per element in `res`), then lz77_walk_kernel as behind the sort.  The caller fills
// blocks[b].ht_bits / min_match2 / ins_end / nkeys / key_off / idx_bits / idx_off; nkeys, nidx: the sums of the blocks' keys and
// index entries (2^idx_bits + 1 each).  ws: lzh_workspace_bytes(total, nkeys, nidx) bytes of device memory.
size_t lzh_workspace_bytes(uint64_t total, uint64_t nkeys, uint64_t nidx);
hipError_t launch_hash_parse(const uint8_t* in_all, const LzBlock* blocks, uint32_t nblocks, uint64_t total, uint64_t nkeys, uint64_t nidx, void* ws,
                             size_t ws_bytes, void* res, LzTok* toks, uint32_t* counts, hipStream_t st, const LzCodes* codes = nullptr);
// LZBuffer's codes from the lists the walk leaves (device/lz77_codes_kernel.h).  Block b owns the item slots tok_off + b ..
// tok_off + b + tok_cap (one per token slot and one for the end of the block); nslots = their number over the batch.
//   pos     nslots + 1 words of 64 bits: every item's length in bits, then (in place) its offset in the batch
//   tmp     lzc_scan_bytes(nslots) bytes for the scan
//   sizes   nblocks + 1 words: every block's stream length in bytes, then the error word (zeroed by the caller; not 0: a list
//           emit_tokens refuses, or more tokens than slots -- then nothing may be emitted)
// launch_lz77_code_lengths runs behind the walk (both launchers above take `codes` and do that); the caller reads `sizes`, places
// the streams -- out_off[b] = block b's first byte in `out`, a multiple of 4, out_off[nblocks] = the end of the last one's room;
// nblocks + 1 words on the device -- zeroes `out` and calls launch_lz77_emit.
size_t lzc_scan_bytes(uint64_t nslots);
hipError_t launch_lz77_code_lengths(const LzBlock* blocks, uint32_t nblocks, const LzTok* toks, const uint32_t* counts, const LzCodes& c, hipStream_t st);
hipError_t launch_lz77_emit(const uint8_t* in_all, const LzBlock* blocks, uint32_t nblocks, uint64_t total, const LzTok* toks, const uint32_t* counts,
                            const LzCodes& c, const uint64_t* out_off, uint8_t* out, hipStream_t st);
// LZ77 streams back into their blocks (device/lz77_decode_kernel.h): launch_unlz_parse leaves 16-byte tokens (stream b's from
// toks + streams[b].tok_off, at most tok_cap) and res[b] = {out_len, ntok, status}; the caller reads res, places the outputs --
// out_off[b] = stream b's first byte in out_all, nstreams words on the device -- and calls launch_unlz_copy, which writes the
// out_len bytes of every stream whose status is 0 and nothing else.
hipError_t launch_unlz_parse(const uint8_t* in_all, const UnlzStream* streams, uint32_t nstreams, void* toks, UnlzResult* res, hipStream_t st);
hipError_t launch_unlz_copy(const uint8_t* in_all, const UnlzStream* streams, uint32_t nstreams, const void* toks, const UnlzResult* res,
                            const uint64_t* out_off, uint8_t* out_all, hipStream_t st);
// ... streams parsed in pieces (device/lz77_decode_wide_kernel.h; the arrays as layout.h UnlzWideStream places them: prov, states
// and fin hold a slot per stream byte rounded up to whole pieces).  launch_unlz_wide_parse leaves the final 16-byte tokens in fin
// and outs[b] (layout.h UnlzWideOut: where err is not all ones its low three bits are the stream's status).  The caller places the outputs of the decoded, non-empty streams back to back (place, in
// the order of the outputs; at most 2^31 bytes) and calls launch_unlz_wide_link, launch_unlz_wide_jump with a zeroed flag word per
// round until a round leaves its flag zero (kUnlzWideRounds at the most), and launch_unlz_wide_emit.
hipError_t launch_unlz_wide_parse(uint32_t level, const uint8_t* in_all, const UnlzWideStream* streams, uint32_t nstreams, const UnlzWideRef* refs, uint32_t npieces,
                                  uint32_t piece, void* prov, uint32_t* states, UnlzWidePieceOut* pieces, void* fin, UnlzWideAdopt* adopt, UnlzWideOut* outs,
                                  hipStream_t st);
hipError_t launch_unlz_wide_link(const uint8_t* in_all, const UnlzWideStream* streams, const UnlzWidePlace* place, uint32_t nlive, uint32_t total,
                                 const void* fin, uint32_t* w, hipStream_t st);
hipError_t launch_unlz_wide_jump(uint32_t* w, uint32_t total, uint32_t* flag, hipStream_t st);
hipError_t launch_unlz_wide_emit(const uint32_t* w, uint32_t total, uint8_t* out, hipStream_t st);
// ... or, in front of the inverse E8E9 filter, launch_unlz_wide_emit_placed: link and jump as above over the packed outputs, then
// the bytes of stream place[a] at out + dst_off[a] (the caller's offsets, multiples of 16 with the rooms rounded up, as launch_une8_mark
// takes its blocks; the padding is not written).
hipError_t launch_unlz_wide_emit_placed(const uint32_t* w, const UnlzWidePlace* place, const uint64_t* dst_off, uint32_t nlive, uint32_t total, uint8_t* out,
                                        hipStream_t st);
// BWT streams back into their blocks (device/bwt_decode_kernel.h): count, scan, link, rank, offsets and emit for nstreams
// admitted streams (layout.h bwt_stream_admitted) placed as `streams` says -- ntiles tiles of 256 words in hist, a word per node
// in link, nsplit entries of 16 bytes in splitters.  status[b] = 0: out_all + out_off holds stream b's n bytes; 1: its path has
// not n nodes and nothing of it was written.
hipError_t launch_bwt_decode(const uint8_t* in_all, const BwtStream* streams, uint32_t nstreams, uint32_t ntiles, uint32_t nsplit, uint32_t* hist,
                             uint32_t* link, void* splitters, uint32_t* status, uint8_t* out_all, hipStream_t st);
// ... of blocks of 16 MiB and more (device/bwt_decode_wide_kernel.h): the same for streams admitted by bwt_wide_stream_admitted --
// 8 bytes per node in link, and nsplit2 entries of 16 bytes in splitters2, stream b's from sp2_off[b] (bwt_splitters2(n) each).
// Count, link, rank and emit are the bodies above (the last three over BwtNode64); the scan takes four parts of a stream's tiles
// at once, and the splitter list is ranked over its own splitters instead of walked by one lane.
hipError_t launch_bwt_decode_wide(const uint8_t* in_all, const BwtStream* streams, const uint32_t* sp2_off, uint32_t nstreams, uint32_t ntiles,
                                  uint32_t nsplit, uint32_t nsplit2, uint32_t* hist, uint64_t* link, void* splitters, void* splitters2, uint32_t* status,
                                  uint8_t* out_all, hipStream_t st);
// The inverse E8E9 filter over blocks in one device buffer, in place (device/e8e9_kernel.h).  blocks[b] = {off, n, tile_off}: off a
// multiple of 16 with the room behind the block rounded up to 16, ntiles = the sum of e8_tiles(n).  launch_une8_mark leaves in
// cnt (2 * ntiles + 1 words) the exclusive prefix sums of the tiles' seed and break counts and zeroes status[0 .. nblocks); tmp:
// une8_scan_bytes(ntiles) bytes.  The caller reads cnt[ntiles] (the seeds) and cnt[2 * ntiles] (seeds + breaks = the words of
// `list`) and calls launch_une8_walk, which rewrites the blocks; status[b] = 1: a lane gave block b up after max_steps steps, its
// bytes are neither the input nor the output.
size_t une8_scan_bytes(uint32_t ntiles);
hipError_t launch_une8_mark(const uint8_t* buf, const E8Block* blocks, uint32_t nblocks, uint32_t ntiles, uint32_t* cnt, uint32_t* status, void* tmp,
                            size_t tmp_bytes, hipStream_t st);
hipError_t launch_une8_walk(uint8_t* buf, const E8Block* blocks, uint32_t nblocks, uint32_t ntiles, const uint32_t* scan, uint32_t* list,
                            uint32_t nseeds, uint32_t max_steps, uint32_t* status, hipStream_t st);
// The forward E8E9 filter over blocks in one device buffer, in place (device/e8e9_forward_kernel.h).  As the two above, except that
// blocks[b].off is any byte offset and no room is rounded up: the blocks lie back to back as the sorters and parsers take them.
// status[b] = 1: a lane gave block b up after max_steps steps, its bytes on the device are neither the input nor the output.
hipError_t launch_e8f_mark(const uint8_t* buf, const E8Block* blocks, uint32_t nblocks, uint32_t ntiles, uint32_t* cnt, uint32_t* status, void* tmp,
                           size_t tmp_bytes, hipStream_t st);
hipError_t launch_e8f_walk(uint8_t* buf, const E8Block* blocks, uint32_t nblocks, uint32_t ntiles, const uint32_t* scan, uint32_t* list,
                           uint32_t nseeds, uint32_t max_steps, uint32_t* status, hipStream_t st);
// The archiver's content-defined fragments (device/fragment_kernel.h): a wavefront per job walks its file in `buf` from job.start
// with a fresh state and appends a record per fragment to recs[job.rec_off ..], until the first cut at or beyond job.stop, a cut
// whose end is in recs[job.merge_off .. + merge_cnt) (ascending ends), or the end of file; res[job] says how it ended.  The
// caller sizes every list with frag_rec_cap (layout.h); a walk that finds no room ends with kFragFull and writes nothing behind it.
hipError_t launch_frag_walk(const uint8_t* buf, const FragJob* jobs, uint32_t njobs, FragParams P, FragRec* recs, FragResult* res, hipStream_t st);
}  // namespace zpq
