// Device-visible data layout shared by the host engine and the HIP kernels.
//
// One in-flight ZPAQ block owns one contiguous ARENA in HBM:
//
//   [ component tables, each 256-B aligned, in COMP order ]   Predictor::init 1776-1846
//   [ H : U32[2^hh] ][ M : U8[2^hm] ][ R : U32[256] ]         ZPAQL::init 1012-1024
//   [ BlockRun : per-block scalar state + h[]/p[] + per-component run vars ]
//
// The plan (parsed header) is immutable and shared by all blocks coded with the
// same header; it lives in its own small device buffer.
#pragma once
#ifndef __HIPCC_RTC__
#include <stdint.h>
#else
// hipRTC has no C library headers; its built-in prelude keeps the fixed-width types in a namespace
using __hip_internal::int8_t;
using __hip_internal::int16_t;
using __hip_internal::int32_t;
using __hip_internal::int64_t;
using __hip_internal::uint8_t;
using __hip_internal::uint16_t;
using __hip_internal::uint32_t;
using __hip_internal::uint64_t;
#endif

namespace zpq {

enum CompType : uint32_t { C_NONE = 0, C_CONS, C_CM, C_ICM, C_MATCH, C_AVG, C_MIX2, C_MIX, C_ISSE, C_SSE };

// How to initialise one arena segment (Predictor::init patterns).
enum FillKind : uint32_t {
  F_ZERO = 0,
  F_U32 = 1,       // every dword = value            (CM 0x80000000, MIX 65536/m, MIX2 0x80008000)
  F_SSE = 2,       // dword j = sse_row[j&31] | value (SSE, value = start count)
  F_ICM = 3,       // copy icm_init[256]
  F_ISSE = 4,      // copy isse_init[512]
  F_MATCHBUF = 5   // zeros, first byte = 1           (MATCH ht(0)=1, libzpaq.cpp:1801)
};

struct Segment {          // 24 bytes
  uint64_t off;           // byte offset in arena (256-B aligned)
  uint64_t bytes;         // multiple of 16
  uint32_t kind;
  uint32_t value;
};

struct CompDesc {         // 64 bytes
  uint32_t type;
  uint32_t a1, a2, a3, a4, a5;   // COMP argument bytes cp[1..5]
  uint32_t limit;         // CM/SSE: cp[]*4 count limit
  uint32_t mask0;         // t0 index mask (elements): CM 2^s-1, MATCH 2^a1-1, MIX/MIX2 2^s-1, SSE 32*2^s-1
  uint32_t mask1;         // t1 mask (bytes): ICM/ISSE ht_n-1, MATCH 2^a2-1
  uint32_t stride;        // MIX: words from one weight row to the next (>= m; see mix_row_stride), 0 otherwise
  uint64_t t0;            // arena offset of cm / a16
  uint64_t t1;            // arena offset of ht
  uint64_t pad1;
};

// MIX weight rows in HBM: row r of an m-input mixer starts at word r * stride.  The reference packs rows (stride = m); a
// row is then 4 m bytes at a 4-byte-aligned address and straddles 128-byte memory lines (m = 19: 76-byte rows, 1.6 lines
// per row on average).  The coder touches one row per bit and component at a random place of a table far larger than any
// cache, and the MI355X's memory system moves 128-byte lines whatever is asked of them (profiles/r03/gups.hip: 49 G
// random line reads per second, 24 G read-modify-writes), so rows are padded to the next power of two up to 32 words:
// one line per row, and 16-byte-aligned for the lane groups that load a row as 16-byte quads.
static inline constexpr uint32_t mix_row_stride(uint32_t m) {
  return m <= 1 ? 1u : (m <= 2 ? 2u : (m <= 4 ? 4u : (m <= 8 ? 8u : (m <= 16 ? 16u : ((m + 31u) & ~31u)))));
}

struct PlanHeader {       // followed in the same buffer by CompDesc[n], Segment[nseg], prog[prog_len]
  uint32_t n;             // components
  uint32_t hmask;         // 2^hh - 1 (elements)
  uint32_t mmask;         // 2^hm - 1 (bytes)
  uint32_t prog_len;      // HCOMP bytes incl. trailing 0
  uint32_t nseg;
  uint32_t wave_ok;       // 1 if the wave-parallel kernel supports this chain
  uint64_t off_H, off_M, off_R, off_run;   // arena offsets
  uint64_t arena_bytes;   // total, 4 KiB multiple
  uint32_t off_comp;      // byte offsets inside this buffer
  uint32_t off_seg;
  uint32_t off_prog;
  uint32_t total_bytes;
  uint64_t dep_mask;      // wave kernel: lanes whose predict needs earlier p[] (ISSE/AVG/MIX2/MIX/SSE)
  uint64_t mix_mask;      // wave kernel: MIX lanes
};

struct SegRange { uint32_t in_begin, in_end, out_end, status; };

// Per-block job descriptor (device array, one per block in the batch).
struct BlockJob {
  const uint8_t* plan;    // -> PlanHeader
  uint8_t* arena;
  const uint8_t* in;
  uint8_t* out;
  uint32_t in_len;
  uint32_t out_cap;       // encode: capacity; decode: max bytes to decode
  uint32_t res_slot;      // index of this block's BlockResult in the results array
  uint32_t nseg;          // 0 / 1: one segment.  > 1: a block of several segments (model and coder state run on,
                          // Compressor::postProcess / Decoder::decompress, libzpaq.cpp:2889-2891, 2129): `segs` has nseg entries
  SegRange* segs;         // encode: in_begin..in_end = the segment's input bytes (consecutive), out_end <- coded bytes so far
                          // decode: in_begin..in_end = the segment's coded bytes incl. terminator, out_end <- decoded bytes so far
};

struct BlockResult {      // 16 bytes
  uint32_t out_len;
  uint32_t consumed;
  int32_t status;
  uint32_t steps;         // coded bits (diagnostic)
};

// Constant tables as uploaded to the device (one buffer).
struct DeviceTables {
  int16_t stretch[32768];
  uint16_t squash[4096];
  int32_t dt[1024];
  int32_t dt2k[256];
  uint8_t ns[1024];
  uint32_t icm_init[256];
  uint32_t isse_init[512];
  uint32_t sse_row[32];
  uint32_t stretch_cb[2016];   // compact stretch (host/common.hpp Tables)
  int16_t stretch_top[256];
};

// One segment to post-process on the device (device/pcomp_kernel.h): the decoded stream after the PP header goes
// through the block's PCOMP program; H, M, R are the program's zeroed work arrays.
struct PcompJob {
  const uint8_t* in;
  uint8_t* out;
  uint8_t* M;
  uint32_t* H;
  uint32_t* R;          // 256 words
  uint32_t in_len, out_cap;
  uint32_t* result;     // [0] bytes produced (may exceed out_cap: then nothing past the capacity was stored), [1] status
};

// One block to hash on the device (sha1_blocks_kernel): digest 20 * slot in the output array.
struct Sha1Job {
  const uint8_t* p;
  uint32_t len;
  uint32_t slot;
};

// Argument block of the pipelined encoder's kernels (device/pipe_kernel.h), passed by value.
struct PipeArgs {
  const BlockJob* jobs;     // the blocks of one plan, consecutive; 64 consecutive blocks form a group
  BlockResult* res;
  uint32_t nblocks;
  const DeviceTables* tb;
  uint8_t* pipe;            // stream + state buffer, PIPE_GROUP_BYTES per group
  int32_t step;             // a unit of dataflow level L works on chunk step - L
  uint32_t wg0;             // added to blockIdx.x: lets a launch cover a sub-range of a kernel's units
  // Placement / timing trace (kernels built with -DZPQ_TRACE, engine run with ZPAQ_AMD_PIPE_TRACE=<file>): four 64-bit
  // words per workgroup and launch, record index = trace_base + blockIdx.x; null otherwise
  unsigned long long* trace;
  uint32_t trace_base;
  uint32_t arrive_need;           // persistent launch: ctl[3] counts the workgroups that have started; a unit begins only when it says
                                  // this many (every workgroup of this launch and of the run's earlier rounds); 0: no handshake
  // The persistent launch (device/pipe_persist.h): one workgroup set per group of blocks for the whole sequence
  uint32_t* prog;                 // progress counters, PS_NUNIT per group, zero at launch
  const uint32_t* group_chunks;   // per group: chunks of its longest block (at least 1)
  uint32_t* ctl;                  // [0] abort flag (zero at launch; 1: a unit's watchdog fired in mid-sequence, 2: the launch's workgroups
                                  // never became resident together -- nothing was touched), [1] the slot whose watchdog fired, [2] its
                                  // chunk, [3] workgroups that have started
  uint32_t group0, ngroups_here;  // the groups this launch serves
  uint32_t timeout_ticks;         // 100 MHz ticks a poller waits without progress before it raises the abort flag
  uint32_t arrive_ticks;          // 100 MHz ticks without a new arrival before a waiting wavefront gives the launch up (flag 2)
  uint32_t spread;                // 8: the workgroups of a group share an XCD (workgroup b of the first 8 * (ngroups / 8) groups serves group
                                  // b % 8 + 8 * (b / 8 / PS_WPG); the other groups' workgroups follow one after the other); 1: group b / PS_WPG
};

// LDS plan of the specialised kernel (spec_kernel.h), known to the host code
// generator: shared constant tables, then one region per wave (block).
static const int kSpecTablesBytes = 32768 + 2688 + 4096 + 512 + 1024;                       // 41088
static const int kSpecLdsBudget = 163840 - 256;                                             // gfx950: 160 KiB per workgroup
// W blocks (waves) per workgroup share the budget: 4 -> 30624 B each, 8 -> 15312 B each
static inline constexpr int spec_wave_lds_bytes(int waves) { return ((kSpecLdsBudget - kSpecTablesBytes) / waves) & ~15; }

// The lockstep decoder (spec_team_kernel.h) keeps 8 blocks' side tables in one workgroup's LDS, so it packs: the compact
// stretch table of the encoder instead of half the full one (8.4 instead of 32 KiB), ICM side-table entries as 16 + 8 bits
// (cm < 2^23), ISSE weight pairs as 2 x 16 + 8 bits (weights are clamped to +-2^19: libzpaq.cpp:2031-2039).  Of the -m5 chain's
// 18 side tables 14 then fit a block's region (7 in the unpacked plan above).
static const int kTeamTablesBytes = 2016 * 4 + 256 * 2 + 2688 + 4096 + 512 + 1024;         // 16896
static inline constexpr int team_block_lds_bytes() { return ((kSpecLdsBudget - kTeamTablesBytes) / 8) & ~15; }   // 18336
static const int kTeamIcmLds = 256 * 2 + 256, kTeamIsseLds = 256 * 4 + 256;                  // 768, 1280 bytes per table

// The pre-processors behind the suffix sort (device/lz77_kernel.h, device/sa_kernels.hip)
struct LzBlock {            // one per block of the batch
  uint64_t off;             // its first element in the batch's arrays (bytes, suffix array, ranks, decisions)
  uint64_t tok_off;         // its first slot in the token array
  uint32_t n;
  uint32_t tok_cap;
  uint32_t kind;            // 1 / 2: LZ77 with bit-packed / byte-aligned codes; 3: BWT; 0: nothing to do here
  uint32_t min_match, lookahead, bucket, checkbits;     // LZBuffer's parameters (args[2], args[6], 2^args[4] - 1, 17 + args[0])
  // the hash-table search (device/lz77_hash_kernel.h); ht_bits == 0: the block is searched through its suffix array
  uint32_t ht_bits;         // args[5]: the table has 2^ht_bits slots (checkbits is 12 - args[0] then)
  uint32_t min_match2;      // args[3]: length of the longer context, 0 = none
  uint32_t idx_bits;        // its index has 2^idx_bits + 1 entries: where the keys of each slot prefix start
  uint32_t nkeys;           // keys of the block: ins_end x (1 or 2)
  uint32_t ins_end;         // positions below max(0, n - minMatchBoth) are inserted, the hashes stand still from there on
  uint32_t rb;              // max(args[0] - 4, 0): low offset bits the bit-packed code writes as they are (device/lz77_codes_kernel.h)
  uint64_t key_off;         // its first key in the batch's key array
  uint64_t idx_off;         // its first entry in the batch's index array
};
struct LzTok { uint32_t i, off, len, blit; };            // = host/common.hpp LzToken
// the error word of the device's coder (device/lz77_codes_kernel.h): a list emit_tokens refuses; more tokens than slots
static const uint32_t kLzcErrList = 1u, kLzcErrCount = 2u;
// The derived fields of a hash-table block (n, min_match, min_match2, lookahead, bucket, ht_bits set; bucket < 2^ht_bits): what
// is inserted, and an index that resolves slot prefixes down to about 8 keys each -- never finer than a bucket, because the slots
// one search reads (h ^ k, k <= bucket) must share their prefix.  nkeys / nidx: running sums over the batch.
static inline void lz_hash_plan(LzBlock& B, uint64_t& nkeys, uint64_t& nidx) {
  const uint32_t ctx2 = B.min_match2 + B.lookahead, both = (B.min_match > ctx2 ? B.min_match : ctx2) + 4u;
  B.ins_end = B.n > both ? B.n - both : 0u;
  B.nkeys = B.ins_end * (B.min_match2 ? 2u : 1u);
  uint32_t bucket_bits = 0, want = 0;
  while ((1u << bucket_bits) <= B.bucket) ++bucket_bits;
  while (want < 24u && (8ull << want) < B.nkeys) ++want;
  const uint32_t most = B.ht_bits > bucket_bits ? B.ht_bits - bucket_bits : 0u;
  B.idx_bits = want < most ? want : most;
  B.key_off = nkeys;
  B.idx_off = nidx;
  nkeys += B.nkeys;
  nidx += (1ull << B.idx_bits) + 1u;
}

// LZ77 streams back into their blocks (device/lz77_decode_kernel.h)
struct UnlzStream {
  uint64_t in_off;       // first byte of the stream in the batch's buffer, a multiple of 4
  uint64_t tok_off;      // first token slot
  uint32_t in_len;       // bytes
  uint32_t tok_cap;      // token slots (in_len: a code has at least 8 bits)
  uint32_t level;        // 1 bit-packed, 2 byte-aligned
  uint32_t rb;           // level 1: low offset bits written as they are
  uint32_t min_match;    // level 2
  uint32_t mbits;        // the program's M holds 2^mbits bytes
};
struct UnlzResult { uint32_t out_len, ntok, status; };

enum { kUnlzOk = 0, kUnlzBefore = 1, kUnlzEmpty = 2, kUnlzLong = 3, kUnlzFull = 4, kUnlzField = 5 };

// ... streams long enough to be parsed in pieces (device/lz77_decode_wide_kernel.h).  A stream of npieces pieces of `piece` bytes
// owns npieces * piece slots from tok_off on in each of three arrays: the pieces' provisional tokens (piece k's from slot
// k * piece), the start states of their codes (4 bytes each, the same slots) and the stream's final list (from slot 0).
static const uint32_t kUnlzWidePiece = 16u << 10;      // bytes of stream per piece
static const uint32_t kUnlzWideRounds = 32;            // jump rounds before the batch is declined
static inline uint32_t unlz_wide_piece_clamped(uint64_t bytes) {      // ZPAQ_AMD_UNLZ_WIDE_PIECE as the engine takes it: [64, 2^20], a multiple of 64
  if (bytes < 64u) bytes = 64u;
  if (bytes > (1u << 20)) bytes = 1u << 20;
  return (uint32_t)((bytes + 63u) & ~63ull);
}
struct UnlzWideStream {
  uint64_t in_off;       // first byte of the stream in the batch's buffer, a multiple of 4
  uint64_t tok_off;      // first slot
  uint32_t in_len;       // bytes
  uint32_t piece0;       // the stream's first piece in the batch's piece tables
  uint32_t npieces;      // (in_len + piece - 1) / piece
  uint32_t level, rb, min_match, mbits;      // as in UnlzStream
  uint32_t pad_;
};
struct UnlzWideRef { uint32_t stream, index; };       // piece g of the batch is piece `index` of stream `stream`
// what the parse of a piece leaves: its list holds `codes` tokens that emit out_len bytes; end 0: it walked out of the piece and
// {exit_pos, exit_t} is the state at the first code start at or behind the piece's end; 1: the stream ended there, as the program
// ends it; 2: the list ends at a code the parser refuses (`status`) -- a verdict only if the true walk gets there
struct UnlzWidePieceOut { uint32_t codes, out_len, exit_pos, exit_t, end, status; };
// what the stitch leaves per piece: tokens first .. first + count of its list are the stream's tokens tok_base .. , and out_base is
// what their positions lack (modulo 2^32)
struct UnlzWideAdopt { uint32_t first, count, tok_base, out_base; };
// ... and per stream: its UnlzResult; err = all ones, or (the first token that fails a check against its absolute position) << 3 |
// the status it declines the stream with, which goes before r.status; the stream's pieces, and how many of them were adopted at
// the state the walk entered them in, met after a serial stretch, walked serially to their end (the rest: a code leapt over them)
struct UnlzWideStats { uint32_t pieces, entered, met, walked; };
struct UnlzWideOut { UnlzResult r; uint32_t pad_; unsigned long long err; UnlzWideStats stats; };
// where a decoded stream's output lies in the batch's (out_len >= 1, ntok tokens in its final list)
struct UnlzWidePlace { uint64_t out_off; uint32_t out_len, ntok, stream, pad_; };

// BWT streams back into their blocks (device/bwt_decode_kernel.h).  A stream is S[0 .. n] and idx in 4 bytes, low byte first.
enum { kBwtTile = 4096, kBwtChunk = 64, kBwtStride = 256 };      // bytes per tile of the counting sort, per step of it, nodes per splitter
struct BwtStream {
  uint64_t in_off;       // S[0] in the batch's buffer, a multiple of 4
  uint64_t link_off;     // the word of node 0 (n + 1 words)
  uint64_t out_off;      // first byte of the output (n bytes, back to back with its neighbours)
  uint32_t n;            // bytes of the block, at least 1
  uint32_t idx;          // 1 .. n, S[idx] == 255: the marker, which is no byte of the block
  uint32_t tile_off;     // first tile: (n + 1 + kBwtTile - 1) / kBwtTile of them, 256 words each
  uint32_t sp_off;       // first splitter: n / kBwtStride + 2 of them (entry 0: node 0, the end; the last: the head, node idx)
};
// what a stream needs of each array (the engine and the emulator's driver place a batch with this)
static inline uint32_t bwt_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + 1u + kBwtTile - 1u) / kBwtTile); }
static inline uint32_t bwt_splitters(uint32_t n) { return n / kBwtStride + 2u; }
// Whether the device takes a stream at all -- everything else is declined before any kernel runs: the rule 1 <= idx <= n and
// S[idx] == 255 (outside it the program's counts and links disagree), n < 2^24 (the node rides in 24 bits of the list's word),
// n + 257 <= 2^mbits (the program's 256 counters sit at the top of H).
static inline bool bwt_stream_admitted(const uint8_t* s, uint64_t len, uint32_t mbits, uint32_t& n, uint32_t& idx) {
  if (len < 6 || len - 5 >= (1ull << 24) || mbits > 32u) return false;
  const uint64_t n64 = len - 5;
  if (n64 + 257u > (1ull << mbits)) return false;
  const uint8_t* t = s + n64 + 1;
  const uint32_t i = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
  if (i < 1u || i > n64 || s[i] != 255u) return false;
  n = (uint32_t)n64;
  idx = i;
  return true;
}
static inline bool bwt_stream_empty(const uint8_t* s, uint64_t len) {      // what preprocess_block writes for an empty block
  return len == 5 && s[0] == 255u && !s[1] && !s[2] && !s[3] && !s[4];
}
// The wide form (device/bwt_decode_wide_kernel.h): what the program computes at args[0] 5 .. 11, where the list's word is a full
// position and the byte is read from M.  The same stream, tiles and splitters; a node's word is 8 bytes ((uint64_t)byte << 32 |
// node), and the splitter list is ranked like the node list: every kBwtStride2-th splitter index is a second-level splitter
// (entry 0: splitter 0, the end; the last: the head).  A stream's second-level table starts at sp2_off[stream], an array beside
// the BwtStream table.
enum { kBwtStride2 = 256 };
static inline uint32_t bwt_splitters2(uint32_t n) { return n / ((uint32_t)kBwtStride * (uint32_t)kBwtStride2) + 2u; }
// Whether the wide form takes a stream: the rule, mbits 25 .. 31 (args[0] 5 .. 11), n + 257 <= 2^mbits -- so n <= 2^31 - 257.
static inline bool bwt_wide_stream_admitted(const uint8_t* s, uint64_t len, uint32_t mbits, uint32_t& n, uint32_t& idx) {
  if (len < 6 || mbits < 25u || mbits > 31u) return false;
  const uint64_t n64 = len - 5;
  if (n64 + 257u > (1ull << mbits)) return false;
  const uint8_t* t = s + n64 + 1;
  const uint32_t i = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
  if (i < 1u || i > n64 || s[i] != 255u) return false;
  n = (uint32_t)n64;
  idx = i;
  return true;
}
// What a batch of streams of either form holds on the device and where each stream lies in it: the engine and the emulator's
// driver place a batch with this and with nothing else.
struct BwtNeed {
  uint64_t streams = 0, in_bytes = 0, nodes = 0, tiles = 0, splits = 0, splits2 = 0, room = 0;
  void add(uint32_t n, bool e8) {
    ++streams;
    in_bytes += ((uint64_t)n + 5u + 3u) & ~3ull;               // every stream starts on a word
    nodes += (uint64_t)n + 1u;
    tiles += bwt_tiles(n);
    splits += bwt_splitters(n);
    splits2 += bwt_splitters2(n);
    room += e8 ? (((uint64_t)n + 15u) & ~15ull) : n;           // (e8_room: the filter's blocks start on a lane's 16 bytes)
  }
  // the next stream of the batch, behind those added so far; sp2_off: where its second-level table starts (the wide form's)
  BwtStream place(uint32_t n, uint32_t idx, bool e8, uint32_t* sp2_off = nullptr) {
    const BwtStream S = {in_bytes, nodes, room, n, idx, (uint32_t)tiles, (uint32_t)splits};
    if (sp2_off) *sp2_off = (uint32_t)splits2;
    add(n, e8);
    return S;
  }
  // the bytes of a wide batch counted against the budget: the node words, 1 KiB per tile, the two splitter tables, the tables per
  // stream, the streams and the outputs (each array starts on 256 bytes)
  uint64_t bytes() const {
    return 8u * nodes + 1024u * tiles + 16u * splits + 16u * splits2 + streams * (sizeof(BwtStream) + 8u) + in_bytes + room + 8u * 256u;
  }
};
typedef BwtNeed BwtWideNeed;       // (its name while only the wide form placed with it)
// The sub-batch that starts at admitted stream `from` (n[k]: its bytes): consecutive streams while the outputs stay within
// out_limit and what the batch holds within held_limit.  Returns its end; `from` itself: that stream does not fit alone.
static inline size_t bwt_wide_cut(const uint32_t* n, size_t m, size_t from, uint64_t out_limit, uint64_t held_limit, bool e8) {
  BwtNeed w;
  size_t k = from;
  for (; k < m && k - from < 65535u; ++k) {
    BwtNeed t = w;
    t.add(n[k], e8);
    if (t.room > out_limit || t.bytes() > held_limit) break;
    w = t;
  }
  return k;
}

// The inverse E8E9 filter over blocks that lie in one device buffer, in place (device/e8e9_kernel.h)
enum { kE8Lane = 16, kE8Tile = 4096 };                 // bytes per lane of the mark pass, per workgroup of 256 lanes
static const uint32_t kE8MaxSteps = 1u << 20;          // serial steps after which a lane gives its block up (a safety: declined)
struct E8Block {
  uint64_t off;          // first byte in the buffer, a multiple of kE8Lane; the room behind the block is rounded up to kE8Lane
  uint32_t n;            // bytes
  uint32_t tile_off;     // first tile: e8_tiles(n) of them
};
static inline uint32_t e8_tiles(uint32_t n) { return n ? (uint32_t)(((uint64_t)n + kE8Tile - 1u) / kE8Tile) : 1u; }
static inline uint64_t e8_room(uint64_t n) { return (n + kE8Lane - 1u) & ~(uint64_t)(kE8Lane - 1u); }

// The archiver's content-defined fragments of a batch of files that lie in one device buffer (device/fragment_kernel.h)
struct FragParams {
  uint32_t min_frag, max_frag;   // a cut needs min_frag bytes, max_frag bytes force one (host/fragment.cpp fragment_limits)
  uint32_t thresh;               // a cut where h < thresh: 2^(22 - fragment), 0 = never (fragment > 22)
};
struct FragRec {                 // one fragment as a walk leaves it
  uint32_t end;                  // offset in the file of the first byte behind it
  uint32_t hits;                 // predictions of the order-1 table that held
  uint8_t o1[256];               // the table at the cut
};
struct FragJob {                 // a wavefront's walk
  uint64_t off;                  // the file's first byte in the buffer
  uint32_t n;                    // the file's bytes
  uint32_t start;                // the walk begins here as if a cut lay in front: a fresh state
  uint32_t stop;                 // it ends at the first cut at or beyond this offset (a cut at n goes on to the end of file)
  uint32_t rec_off, rec_cap;     // its list in the record array: first record, room
  uint32_t merge_off, merge_cnt; // a fix-up: the list (ascending ends) of the piece it walks into; it ends at a cut found there
};
enum { kFragStop = 0, kFragEof = 1, kFragMerged = 2, kFragFull = 3 };
struct FragResult {
  uint32_t count;                // records written
  uint32_t status;               // kFragStop: ended at a cut >= stop; kFragEof: the last record is the fragment that ran into the
                                 // end of file; kFragMerged: the last record's end is merge list[merge_at].end; kFragFull: no room
  uint32_t merge_at;
};
// the records a walk from `start` that ends at the first cut >= stop (or at the end of file) can write: a cut needs min_frag bytes
static inline uint64_t frag_rec_cap(uint64_t start, uint64_t stop, uint32_t min_frag) {
  return (stop > start ? stop - start : 0u) / (min_frag ? min_frag : 1u) + 3u;
}

// Cap on HCOMP instructions per input byte: the reference has no limit (a
// hostile header can loop forever); a device kernel must not hang.
static const uint32_t kMaxVmSteps = 1u << 20;

}  // namespace zpq
