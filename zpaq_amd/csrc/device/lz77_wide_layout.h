// What the host and the kernels share of the LZ77 parse of one block in pieces (device/lz77_wide_kernel.h).
#pragma once
#include <stdint.h>

namespace zpq {

// The walk of ONE block in pieces (device/lz77_wide_kernel.h).  Piece k covers [k piece, (k + 1) piece) and owns the slot_cap
// token slots from k slot_cap of the provisional array.
struct LzWideParams { uint32_t n, piece, npieces, slot_cap; };
struct LzWidePiece { uint32_t count, exit_i, exit_lit, pad; };      // lz77_wide_walk: tokens listed, the state the walk left the piece in
// lz77_wide_stitch per piece: the provisional tokens [first, first + count) go to dst .. of the final list; how = kLzWide...
struct LzWideAdopt { uint32_t first, count, dst, how; };
static const uint32_t kLzWideWhole = 0u, kLzWideRejoined = 1u, kLzWideOwn = 2u;     // adopted whole; re-walked, then re-joined; re-walked tokens only, or nothing
// ... and for the block: the final count (may exceed the list's slots: incomplete then), the pieces by `how`, and whether some
// piece's own list was incomplete (never, by the slot count: checked all the same)
struct LzWideResult { uint32_t count, pieces, how[3], overflow, pad[2]; };
static inline uint32_t lz_wide_slot_cap(uint32_t piece, uint32_t min_match) { return piece / (min_match ? min_match : 1u) + 2u; }
// ZPAQ_AMD_LZ_WIDE_PIECE as the engine takes it: [64, 2^30], a multiple of 64
static inline uint32_t lz_wide_piece_clamp(uint64_t bytes) {
  const uint64_t p = bytes < 64u ? 64u : (bytes > (1ull << 30) ? (1ull << 30) : bytes);
  return (uint32_t)((p + 63u) & ~63ull);
}
static const uint32_t kLzWidePiece = 1u << 16;      // a multiple of the flush (4096): data without matches is adopted whole

}  // namespace zpq
