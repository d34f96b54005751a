#pragma once
#include <vector>

#include "../host/common.hpp"
#include "layout.h"
#include "plan.hpp"

namespace zpq {

struct HostBlock {
  const zpq_plan* plan;
  const U8* prefix;   // optional bytes coded before `in` (the PP header), may be null
  U32 prefix_len;
  const U8* in;
  U32 in_len;
  U8* out;        // host destination (may be null to discard)
  U32 out_cap;    // encode: capacity; decode: max bytes to decode
  // A block of several segments (model and coder state run on from one to the next): nseg > 1, seg_len[s] = the
  // segment's share of `in` (encode: input bytes, the prefix belongs to the first; decode: coded bytes incl. its
  // terminator), seg_out_end[s] <- where the segment's output ends in `out`.  Pipelined encoder / wavefront decoder only.
  U32 nseg = 0;
  const U32* seg_len = nullptr;
  U32* seg_out_end = nullptr;
  U8* sha1_out = nullptr;   // encode: if set, SHA-1 of `in` (without the prefix) is computed on the device into these 20 bytes
};

struct Timing {
  float init_ms = 0;   // init_arena_kernel (Predictor::init)
  float code_ms = 0;   // coding kernel(s)
  uint32_t blocks = 0;
};

void engine_init(int device);
// contiguous share [lo, hi) of n blocks for shard k of `parts` (how host batches are split over devices)
void engine_shard_range(uint64_t n, uint32_t parts, uint32_t k, uint64_t* lo, uint64_t* hi);
int engine_device_count();
int engine_count();                      // engines configured by zpq_init (one per device named; a device may be named twice)
void engine_shutdown();
void engine_set_budget(uint64_t bytes);
void engine_set_kernel(int which);
Timing engine_last_timing();
bool engine_last_persistent();
double engine_last_persist_abort_ms();
void engine_plan_release(zpq_plan* p);
// 4 pipelined encoder (compression only) / 3 specialised / 2 generic wave / 1 generic one-lane; note = origin of the specialised kernel or why not
int engine_plan_kernel_kind(zpq_plan* p, std::string& note, bool decode = false, uint32_t nblocks = 0, uint32_t block_bytes = 0);   // nblocks = 0: a batch that fills the GPU

// Host-buffer batch: copies in, runs (possibly in several residency waves), copies out.  Concurrent callers are
// coalesced into one device batch (see the submission queue in engine.cpp); a caller that will submit shortly
// announces itself with engine_caller_enter() and withdraws the announcement with engine_caller_leave() right
// before it submits (or gives up), so that the batch leader waits for it.
// announced = the caller called engine_caller_enter() before: the announcement is withdrawn once its blocks are queued
void engine_code_host(bool decode, const std::vector<HostBlock>& blocks, std::vector<BlockResult>& results,
                      bool* announced = nullptr);
void engine_caller_enter();
void engine_caller_leave();

// Device-resident batch; plans[0] for every block when one_plan, else plans[b] per block.  Results
// land in the device array d_res in the caller's block order.
void engine_code_device(bool decode, const zpq_plan* const* plans, bool one_plan, const void* d_in,
                        const uint64_t* in_off, const uint32_t* in_len, uint32_t nblocks, void* d_out,
                        const uint64_t* out_off, const uint32_t* out_cap, BlockResult* d_res, void* stream, bool timed);

// Post-processing on the device: every segment's stream (decoded bytes after the PP header) through its block's PCOMP
// program, one lane per segment.  Returns false (note says why) when the program cannot run there: the caller then
// uses the host interpreter.  out[i] receives segment i's data; hint[i] = expected size or 0.  *handed_back (when given) tells
// the two kinds of false apart: true when the kernel exists and the SEGMENTS go back to the host (a device status, an output
// beyond the kernel's 32-bit range, the device budget), false when the program has no kernel here.
struct PcompSeg { const U8* in; U32 in_len; U64 hint; std::vector<U8>* out; };
bool engine_pcomp(const U8* code, size_t codelen, int ph, int pm, std::vector<PcompSeg>& segs, std::string& note, bool* handed_back = nullptr);
void engine_sha1_host(const uint8_t* const* in, const uint32_t* len, uint32_t n, uint8_t* out);
// Suffix arrays of host buffers, all in one device call (device/sa_kernels.hip: prefix doubling over the whole batch).
// false + note when the device declines (then the host sorts): a buffer of 2^24 bytes or more, too many buffers, memory.
bool engine_suffix_arrays(const std::vector<std::pair<const U8*, U32>>& blocks, std::vector<std::vector<U32>>& sa, std::string& note);
// The pre-processors behind the sort for a whole batch on the device (device/lz77_kernel.h): blocks of kind 1 / 2 come back as
// the LZ77 parse's list of matches (host/preproc.cpp lz77_serialize codes it), blocks of kind 3 as the BWT stream
// preprocess_block would make (n + 5 bytes).  false + note when the device declines (then the host does it all).
// codes: LZBuffer's codes are written on the device as well (device/lz77_codes_kernel.h) -- a block of kind 1 / 2 then comes back
// as its finished stream in SortOut::codes (coded = true) and its list of matches is not downloaded.
// e8 (null: the caller has filtered already, or the method has no E8E9): filter this block there.  `data` is then the unfiltered
// block in a buffer the caller lets be written, and the stage runs device/e8e9_forward_kernel.h over the uploaded copy before
// anything else reads it.  *e8 says what `data` holds, also when the stage returns false or throws: kE8Not the unfiltered bytes
// still; kE8Device the filtered bytes, downloaded; kE8Host the filtered bytes, made by e8e9_forward here because the device
// declined the block (a walk beyond the step cap, the list beyond the budget, a failed launch) and uploaded over the copy;
// kE8InFlight a download that failed -- the buffer is in no known state and the caller must pass the error on.
enum : U8 { kE8Not = 0, kE8Device = 1, kE8Host = 2, kE8InFlight = 3 };
struct SortJob { const U8* data; U32 n; U32 kind, min_match, lookahead, bucket, checkbits; U32 min_match2 = 0, ht_bits = 0, rb = 0; U8* e8 = nullptr; };   // (min_match2, ht_bits: hash_job; rb: the coder)
// The forward E8E9 filter on its own for n host buffers, in place (device/e8e9_forward_kernel.h): one upload, the filter, the
// buffers with status 0 down again.  status[b] = 1: declined after max_steps serial steps (0: kE8MaxSteps), data[b] untouched.
// false + note: outside the range (65 535 buffers, 2 GiB per batch, the device budget), nothing touched.
bool engine_e8e9_device(U8* const* data, const U32* len, U32 n, U32 max_steps, int32_t* status, std::string& note);
// Whether a batch of the suffix-sort or hash-parse route (blocks, bytes: its E8E9 blocks) / a wide block of n bytes is filtered on
// the device when ZPAQ_AMD_DEVICE_E8 is unset.  The rule is that of sa_wide_pays: from the smallest measured size at which the
// device filter won every alternation on every kind of data; false wherever nothing was measured.
inline bool e8_forward_pays(U64 /*blocks*/, U64 /*bytes*/) { return false; }
inline bool e8_forward_wide_pays(U64 /*n*/) { return false; }
struct SortOut { std::vector<LzToken> toks; std::vector<U8> bwt; std::vector<U8> codes; bool coded = false; std::vector<U32> sa; bool parsed = false; };   // (sa, parsed: engine_sort_wide)
// codes: 0 the lists come back; 1 the streams; 2 the streams when that pays -- decided per batch once the sizes are known, by
// lz_codes_pay below (DESIGN 4.5.2 has the measurement behind it)
bool engine_sort_preprocess(const std::vector<SortJob>& jobs, std::vector<SortOut>& out, std::string& note, int codes = 0);
// The device writes the codes of a batch whose streams are smaller than its lists (16 bytes per match: less comes back over PCIe
// and no host core walks the blocks) unless they are below 1 % of the input (long repeats: either way moves next to nothing, and
// no gain was measured).  An incompressible batch has no matches: its list is empty, its stream is the input.
inline bool lz_codes_pay(U64 matches, U64 stream_bytes, U64 input_bytes) { return 16 * matches > stream_bytes && 100 * stream_bytes >= input_bytes; }
inline U32 lz_offset_rb(const int args[9]) { return args[0] > 4 ? (U32)(args[0] - 4) : 0u; }     // low offset bits level 1 writes as they are
// the job of a block whose method has these args (LZBuffer's parameters: libzpaq.cpp:6647-6692)
inline SortJob sort_job(const U8* data, U32 n, const int args[9]) {
  const U32 level = (U32)(args[1] & 3);
  if (level == 3) return SortJob{data, n, 3u, 0u, 0u, 0u, 0u};
  SortJob j{data, n, level, (U32)args[2], (U32)args[6], args[4] >= 0 && args[4] < 31 ? (1u << args[4]) - 1u : 0x7FFFFFFFu, (U32)(17 + args[0])};
  j.rb = lz_offset_rb(args);
  return j;
}
// ONE block of any length below 2^31 through the wide sorter (device/sa_wide_kernel.h, DESIGN 4.5.7: no block id in the key, two
// rank fields of up to 31 bits).  A block of kind 3 comes back as its BWT stream in out.bwt (n + 5 bytes, emitted on the device
// from the ranks) unless want_sa.  A block of kind 1 / 2 with parse_codes >= 0 and not want_sa is parsed there as well, in pieces
// (device/lz77_wide_kernel.h, DESIGN 4.5.9: n < 2^31, min_match >= 1, lookahead <= 255, 1 <= checkbits <= 31, rb <= 7) and comes
// back with out.parsed set, as its list of matches in out.toks or -- parse_codes 1, or 2 and lz_codes_pay -- as its stream in
// out.codes (coded = true), exactly as a batch's blocks do.  Every other block, every block with want_sa, and a block whose sort
// fits the budget but whose parse does not, or whose parse failed (an overflowed list, one the coder's checks refuse, a launch
// error: the note says), comes back as its suffix array in out.sa -- the host parses or transforms with it.  false + note when
// the device declines (the block, its array or column and 32 bytes of workspace per byte within the engine's budget): nothing was
// launched, the host sorts.
// parse_or_nothing: the caller wants the parse and has no use for the array -- where the parse cannot run (the range, the budget)
// the call declines before anything is launched.
bool engine_sort_wide(const SortJob& job, SortOut& out, std::string& note, bool want_sa, int parse_codes = -1, bool parse_or_nothing = false);
// What such a call holds on the device -- the sums its budget check makes: out[0] the sort alone, out[1] the sort with the parse
// and the coder's arrays behind it (equal for a block that is not parsed there).  Needs no device.  ZPAQ_AMD_LZ_WIDE_PIECE=<bytes>,
// read per call, overrides the piece size (kLzWidePiece; clamped to [64, 2^30], rounded up to a multiple of 64: tests).
void engine_wide_stage_bytes(const SortJob& job, U64 out[2]);
// pieces of this process's last wide parse: all, adopted whole, re-joined after a re-walk, own tokens only or nothing
void engine_last_wide_parse_pieces(U32 out[4]);
// Whether the parse of a wide LZ77 block runs on the device when ZPAQ_AMD_DEVICE_PARSE_WIDE is unset.  The rule is that of
// sa_wide_pays, fixed before the measurement: from the smallest measured block size at which the device parse beat the host's
// in all three alternations on every kind of data, never below 2^24 bytes; off, behind the knob only, if some kind loses at every
// size.  Zeros do: 381 against 105 ms at 16 MiB + 4096, 1511 against 476 ms at 64 MiB - 4096 (the search compares a run's 49 152
// bytes at every position) -- while text, records and random bytes are parsed 14 to 55 times faster (DESIGN 4.5.9 has the table).
inline bool lz_wide_parse_pays(U64 /*n*/) { return false; }
U32 engine_last_wide_sort_rounds();    // doubling rounds of this process's last engine_sort_wide call that sorted
// Whether a sorting block of n bytes takes the wide route when ZPAQ_AMD_DEVICE_SORT_WIDE is unset.  The rule, fixed before the
// measurement: from the smallest measured block size at which the route beat the host's sorter in all three alternations on
// every kind of data, never below 2^24 bytes.  That size is the smallest one measured, 16 MiB + 4096: 20 to 49 times faster
// end to end on text, records and random bytes, 1.7 to 2.1 times on zeros (26 rounds), at every size up to 64 MiB - 4096
// (DESIGN 4.5.7 has the table).
inline bool sa_wide_pays(U64 n) { return n >= (16ull << 20) + 4096; }
// The LZ77 parse through LZBuffer's hash table (args[5] - args[0] < 21: method 1, method 2 below type 64, ...) for a whole batch on
// the device (device/lz77_hash_kernel.h): every block comes back as its list of matches, like the kind 1 / 2 blocks of
// engine_sort_preprocess.  Same buffers, same contract: false + note when the device declines or fails (then the host parses),
// nothing of the caller's is touched.
bool engine_hash_preprocess(const std::vector<SortJob>& jobs, std::vector<SortOut>& out, std::string& note, int codes = 0);
inline SortJob hash_job(const U8* data, U32 n, const int args[9]) {
  SortJob j{data, n, (U32)(args[1] & 3), (U32)args[2], (U32)args[6], args[4] >= 0 && args[4] < 31 ? (1u << args[4]) - 1u : 0x7FFFFFFFu, (U32)(12 - args[0])};
  j.min_match2 = (U32)args[3];
  j.ht_bits = (U32)args[5];
  j.rb = lz_offset_rb(args);
  return j;
}
// What the device's hash-table parser takes (everything else stays on the host): blocks below 2^24 bytes, tables of up to 2^24
// slots that hold a whole bucket, a look-ahead the decision word has room for, and min_match >= 2 -- with 1 the reference
// compares the byte in front of a candidate, which for position 0 lies outside the block.  Level 2 with min_match > 64 searches
// nothing in the reference.
inline bool hash_job_in_range(const SortJob& j) {
  return (j.kind == 1 || j.kind == 2) && j.n < (1u << 24) && j.ht_bits >= 1 && j.ht_bits <= 24 && j.bucket < (1u << j.ht_bits) && j.lookahead <= 255 &&
         j.min_match >= 2 && j.min_match <= 255 && j.min_match2 <= 255 && (j.kind == 1 || j.min_match <= 64) && j.checkbits >= 1 && j.checkbits <= 12;
}
// LZBuffer's codes for given token lists over given (already filtered) blocks, on the device: what host/preproc.cpp
// lz77_serialize writes, list by list.  1: out[i] holds stream i; 0: some list is one emit_tokens refuses (nothing is emitted);
// -1 + note: the device declines (blocks of 2^24 bytes and more, more than 65 535 blocks, 2 GiB per batch, memory).
struct CodeJob { const U8* data; U32 n, kind, min_match, rb; const LzToken* toks; size_t ntok; };
int engine_lz77_codes(const std::vector<CodeJob>& jobs, std::vector<std::vector<U8>>& out, std::string& note);
// One stream of a batch the device decodes back into its block (engine_lz77_decode, engine_bwt_decode, engine_e8e9_decode): the
// output goes to `vec` (resized) when set, else to out[0..cap).  status 0: decoded, out_len bytes; 1: declined, the output untouched --
// the device never gives a verdict on a stream, the caller's other route does.  The three calls return 1: done, status / out_len
// per job; 0: some decoded block does not fit its cap -- every out_len is reported, nothing is written; -1 + note: the device
// declines the batch.
struct StreamJob { const U8* in; U32 in_len; U8* out; U64 cap; std::vector<U8>* vec; U64 out_len = 0; int status = 1; };
// LZ77 streams of one method back into their blocks on the device (device/lz77_decode_kernel.h): what the method's PCOMP program
// (level 1 / 2 without E8E9; rb = lz_offset_rb, mbits = the program's pm) makes of each stream.  The batch is declined
// (-1 + note) beyond 65 535 streams, 2 GiB of output, or the engine's budget.
int engine_lz77_decode(U32 level, U32 rb, U32 min_match, U32 mbits, std::vector<StreamJob>& jobs, std::string& note);
// Whether a group of qualifying segments takes that route when ZPAQ_AMD_DEVICE_UNLZ is unset: from the smallest batch at which
// it was faster than both other routes (the translated program on the device, a lane per segment; the host's translated
// programs) in every alternation of the measurement -- 256 segments of 1 MiB (DESIGN 4.5.3 has the table and the rule).
inline bool lz_unlz_pays(U64 segments, U64 /*stream_bytes*/) { return segments >= 256; }
// The same streams through the decoder that parses a stream in pieces and copies by pointer jumping (device/lz77_decode_wide_kernel.h,
// DESIGN 4.5.10), for streams long enough to be cut: the same contract per stream, 1 / 0 / -1 as StreamJob says.  The pieces'
// tokens, the final list and the start states (36 bytes per stream byte, rounded up to whole pieces), 4 bytes per output byte, the
// streams and the outputs count against the engine's budget; at most 65 535 streams, outputs below 2^31 bytes.  Jobs that all
// deliver into vectors are cut into sub-batches that fit, and only a stream that does not fit alone is declined (status 1; -1 +
// note when nothing else was decoded); jobs with buffers of their own run as one batch or are declined (-1 + note).
// ZPAQ_AMD_UNLZ_WIDE_PIECE=<bytes>, read per call, overrides the piece size (kUnlzWidePiece; clamped to [64, 2^20], rounded up to a
// multiple of 64: tests).
int engine_lz77_decode_wide(U32 level, U32 rb, U32 min_match, U32 mbits, std::vector<StreamJob>& jobs, std::string& note);
// pieces of this process's last engine_lz77_decode_wide call: all, adopted in the state the walk entered them in, met after a
// serial stretch, walked serially to their end (the rest: a code leapt over them); and the jump rounds of its longest copy
void engine_last_unlz_wide_pieces(U32 out[4]);
U32 engine_last_unlz_wide_rounds();
// Whether the segments of a group whose streams are long enough (host/blocks.cpp: ZPAQ_AMD_UNLZ_WIDE_FROM) take that route when
// ZPAQ_AMD_DEVICE_UNLZ_WIDE is unset.  The rule is the one of lz_unlz_pays, fixed before the measurement: from the smallest
// measured stream size at which the route beat both other settings in all three alternations on every kind of data; off, behind
// the knob only, if the kinds disagree.  Off while the measurement is incomplete, and it is: the 16 MiB class is timed (the route won on text, records and random
// bytes), the 64 MiB class in part only (DESIGN 4.5.10 has the table).
inline bool lz_unlz_wide_pays(U64 /*segments*/, U64 /*stream_bytes*/) { return false; }
// BWT streams back into their blocks on the device (device/bwt_decode_kernel.h): what the program of a BWT method without E8E9
// at args[0] <= 4 (mbits = the program's pm = ph) makes of each stream, or status 1: declined, the output untouched -- a stream
// outside the rule 1 <= idx <= n, S[idx] == 255 or shorter than 5 bytes, n >= 2^24, n + 257 > 2^mbits, a path that has not n
// nodes.  The device never gives a verdict on a stream.  Sizes are known before any kernel runs (n = in_len - 5), so:
// 1: done, status / out_len per job; 0: some admitted stream does not fit its cap -- every out_len is reported, nothing is
// launched or written; -1 + note: the device declines the batch (more than 65 535 streams, 2 GiB of output, memory: 4 bytes per
// stream byte, the tile histograms, the splitter tables and the outputs count against the engine's budget).
int engine_bwt_decode(U32 mbits, std::vector<StreamJob>& jobs, std::string& note);
// Whether a group of qualifying segments takes that route when ZPAQ_AMD_DEVICE_UNBWT is unset.  The rule is the one of
// lz_unlz_pays, fixed before the measurement: from the smallest measured group at which the route beat both other settings in
// all three alternations, never below 64 segments, off while no measurement exists.  No measurement exists.
inline bool bwt_unbwt_pays(U64 /*segments*/, U64 /*stream_bytes*/) { return false; }
// The same for the program at args[0] 5 .. 11 (mbits 25 .. 31; device/bwt_decode_wide_kernel.h): the list's word is
// a full position, so n goes up to 2^31 - 257; e8: the method is xN,7 and the inverse E8E9 filter runs over the outputs while
// they are on the device, as for kind 7 of engine_e8e9_decode.  1 / 0 / -1 as for engine_bwt_decode, but a batch whose outputs
// exceed 2 GiB or whose workspace (8 bytes per stream byte for the list, 1 KiB per tile, the two splitter tables, the streams
// and the outputs) exceeds the budget is cut into consecutive sub-batches that each fit; only a stream that does not fit alone
// is declined (status 1; -1 + note when nothing else was decoded).
int engine_bwt_decode_wide(U32 mbits, bool e8, std::vector<StreamJob>& jobs, std::string& note);
// Whether a group of qualifying xN,3 segments takes that route when ZPAQ_AMD_DEVICE_UNBWT is unset.  The
// rule is the one of lz_unlz_pays, fixed before the measurement: from the smallest measured group size (bytes of admitted
// output) at which the route beat both other settings in all three alternations (DESIGN 4.5.8 has the table).  That is the
// smallest size measured, one block of 2^24 + 4 097 bytes: 17 ms against 2.2 s for the host's program and 18 s for the one-lane
// kernel on text.  Groups below it were not measured and stay with the route they had unless the knob says 1.
inline bool bwt_unbwt_wide_pays(U64 /*segments*/, U64 stream_bytes) { return stream_bytes >= (1ull << 24) + 4097; }
// The same for xN,7 groups and ZPAQ_AMD_DEVICE_UNE8, by the same rule.  No xN,7 group has been timed -- neither the filter behind
// the wide stage nor the windowed program it replaces -- so the route is off unless the knob says 1.
inline bool bwt_une8_wide_pays(U64 /*segments*/, U64 /*stream_bytes*/) { return false; }
// Streams of the E8E9 methods back into their blocks on the device: kind = args[1], 5 / 6 the LZ77 decoder of level 1 / 2 (rb,
// min_match, mbits as for engine_lz77_decode), 7 the BWT decoder (mbits as for engine_bwt_decode), 4 nothing -- then the inverse
// filter over the stage's output while it is on the device (device/e8e9_kernel.h: candidates, seeds and breaks marked from the
// original bytes, a lane per chain's first seed walks it), then the blocks down.  What the method's program makes of each stream,
// or status 1: declined, the output untouched -- whatever the stage in front declines (an output beyond 2^mbits among it: the
// programs filter M, which wraps there), and a block in which a lane gave up after kE8MaxSteps serial steps.  1 / 0 / -1 as
// StreamJob says (kinds 4 and 7 know every size before anything runs); 65 535 streams and 2 GiB of output per batch; the
// tiles' counts and the list of seeds and breaks (4 bytes each) count against the engine's budget.
int engine_e8e9_decode(int kind, U32 rb, U32 min_match, U32 mbits, std::vector<StreamJob>& jobs, std::string& note);
// Whether a group of qualifying segments takes that route when ZPAQ_AMD_DEVICE_UNE8 is unset.  The rule is the one of
// lz_unlz_pays, fixed before the measurement: from the smallest measured group at which the route beat both other settings in
// all three alternations, never below 64 segments, off while no measurement exists.  No measurement exists.
inline bool e8_une8_pays(U64 /*segments*/, U64 /*stream_bytes*/) { return false; }
// Streams of the methods x.,5 and x.,6 (kind; anything else: -1 + note) through the decoder that parses a stream in pieces, then
// the inverse filter: engine_lz77_decode_wide with level = kind - 4, its outputs emitted into rooms placed for
// device/e8e9_kernel.h -- each on a multiple of 16 bytes, rounded up to one -- and filtered there before they go down.  The
// contract per stream is engine_e8e9_decode's; 1 / 0 / -1, the sub-batches and ZPAQ_AMD_UNLZ_WIDE_PIECE as for
// engine_lz77_decode_wide, whose counters (engine_last_unlz_wide_pieces, engine_last_unlz_wide_rounds) report this call too.  The
// rooms' padding, the tiles' counts and the list of seeds and breaks count against the budget besides what that decoder holds;
// the 2 GiB are of the rooms.  An empty output never enters the filter's list.
int engine_e8e9_decode_wide(int kind, U32 rb, U32 min_match, U32 mbits, std::vector<StreamJob>& jobs, std::string& note);
// Whether the segments of an x.,5 / x.,6 group whose streams are long enough (host/blocks.cpp: ZPAQ_AMD_UNLZ_WIDE_FROM) take that
// route unless ZPAQ_AMD_DEVICE_UNE8 and ZPAQ_AMD_DEVICE_UNLZ_WIDE both say 1.  The rule is the one of lz_unlz_wide_pays, fixed
// before the measurement: from the smallest measured stream size at which the route beat both other settings in all three
// alternations on every kind of data.  Off: no default rests on a measurement of this shape yet (DESIGN 4.5.10 has the table).
inline bool e8_unlz_wide_pays(U64 /*segments*/, U64 /*stream_bytes*/) { return false; }
// The archiver's content-defined fragments of a batch of files on the device (device/fragment_kernel.h): the files
// are uploaded and divided into pieces of kFragPiece bytes, or 64 smallest fragments where that is more (ZPAQ_AMD_FRAG_PIECE, in
// bytes, read per call, overrides both: tests).
// Round 0 walks every piece from its own start as if a cut lay there.  Then the host stitches: the true start of a piece is the
// last cut of the accepted list of the piece in front; where that is not the piece's own start a fix-up walks from it until one
// of its cuts is in the piece's list -- from there the list is the truth -- or until it has passed the piece's end.  The fix-ups
// of all pieces run in one launch per round on provisional starts (the last cuts of the lists as they stand); the host accepts
// pieces in order while their starts were the true ones, the rest run again.  The first open piece of a file always has its true
// start, so every round finishes a piece: data that never re-joins (constant bytes) degenerates to a serial walk and stays
// exact.  Then one SHA-1 job per fragment (launch_sha1).  out[f] = the fragments of file f, exactly fragment_scan's.
// 1 done; -1 + note: outside the range (65 535 files and 2 GiB of input per batch; the files and twice the worst-case record
// lists, 264 bytes per min_frag bytes, within the engine's budget) -- nothing was delivered.
static const U32 kFragPiece = 1u << 18;        // 256 KiB: 36 against 47 ms with 1 MiB on one file of 256 MiB
int engine_fragment(const U8* const* in, const U64* len, U32 n, const FragLimits& lim, std::vector<std::vector<Fragment>>& out, std::string& note);
U32 engine_last_fragment_rounds();     // fix-up rounds of this process's last engine_fragment call (0: every piece began at a cut)
int engine_selftest(int32_t out[8]);
int engine_jit_threads();      // host threads spec_precompile() uses by default (the host cores the process may use, at most 16)

}  // namespace zpq
