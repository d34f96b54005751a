// The engine's batch stages of the compression side: SHA-1 of host buffers, the suffix sort, the pre-processors behind it and
// through the hash table, LZBuffer's codes, the archiver's fragments.  Each takes the engine for one call (EngineCall), sums what
// its batch holds on the device against the engine's budget, stages its inputs, launches, and delivers or declines.
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdlib>

#include "../host/common.hpp"
#include "engine_internal.hpp"
#include "fragment_stitch.hpp"
#include "kernels.h"
#include "sa_kernels.h"

namespace zpq {

// SHA-1 of ranges that lie on the device, one lane per job: the jobs up, the kernel, 20 bytes per job down into `out`
static void sha1_round_trip(Engine& e, const std::vector<Sha1Job>& jobs, uint8_t* out) {
  const size_t n = jobs.size();
  e.sha_jobs.ensure(n * sizeof(Sha1Job));
  e.sha_out.ensure(n * 20);
  HIP_CHECK(hipMemcpyAsync(e.sha_jobs.p, jobs.data(), n * sizeof(Sha1Job), hipMemcpyHostToDevice, e.stream));
  HIP_CHECK(launch_sha1((const Sha1Job*)e.sha_jobs.p, (uint32_t)n, (uint8_t*)e.sha_out.p, e.stream));
  HIP_CHECK(hipMemcpyAsync(out, e.sha_out.p, n * 20, hipMemcpyDeviceToHost, e.stream));
  HIP_CHECK(hipStreamSynchronize(e.stream));
}

// SHA-1 of n host buffers on the device (one lane per buffer); 20 bytes each into out.
void engine_sha1_host(const uint8_t* const* in, const uint32_t* len, uint32_t n, uint8_t* out) {
  EngineCall call;
  Engine& e = call.e;
  std::vector<HostItem> items(n);
  uint64_t bytes = 0;
  for (uint32_t i = 0; i < n; ++i) {
    items[i] = HostItem{in[i], len[i], bytes};
    bytes += align_up(len[i], 64);
  }
  e.io_in.ensure(bytes + 64);
  std::vector<Sha1Job> jobs(n);
  for (uint32_t i = 0; i < n; ++i) jobs[i] = Sha1Job{(const uint8_t*)e.io_in.p + items[i].off, len[i], i};
  const auto staged = upload_staged(e, e.io_in.p, items, bytes, 64, false);
  sha1_round_trip(e, jobs, out);
}

// The sorter's inputs of a batch: the blocks back to back in io_in (which holds in_bytes + 64) -- through page-locked memory from
// 1 MiB -- and, in e.jobs, where each starts on the device and, behind that on a 16-byte boundary, the n + 1 offsets.  The host's
// copies live here until the caller has synchronised the stream.
struct SaInputs {
  std::vector<const uint8_t*> ptrs;
  std::vector<uint64_t> off;
  std::unique_ptr<uint8_t[]> staged;
  const uint8_t* const* d_ptrs = nullptr;
  const uint64_t* d_off = nullptr;
};
static void upload_sa_inputs(Engine& e, const std::vector<HostItem>& items, uint64_t total, uint64_t in_bytes, SaInputs& s) {
  const size_t n = items.size();
  e.jobs.ensure((n + 2) * 16 + 64);
  s.ptrs.resize(n);
  s.off.assign(n + 1, total);
  for (size_t i = 0; i < n; ++i) {
    s.ptrs[i] = (const uint8_t*)e.io_in.p + items[i].off;
    s.off[i] = items[i].off;
  }
  uint8_t* meta = (uint8_t*)e.jobs.p;
  s.d_ptrs = (const uint8_t* const*)meta;
  s.d_off = (const uint64_t*)(meta + align_up(n * 8, 16));
  s.staged = upload_staged(e, e.io_in.p, items, total, 0, in_bytes >= (1u << 20));
  HIP_CHECK(hipMemcpyAsync(meta, s.ptrs.data(), n * 8, hipMemcpyHostToDevice, e.stream));
  HIP_CHECK(hipMemcpyAsync(meta + align_up(n * 8, 16), s.off.data(), (n + 1) * 8, hipMemcpyHostToDevice, e.stream));
}

// ---- the forward E8E9 filter (device/e8e9_forward_kernel.h) ----

// the walk's cap on serial steps: kE8MaxSteps, or less with ZPAQ_AMD_E8_MAX_STEPS=<steps>, read per call (tests: a decline
// without a pathological megabyte)
static uint32_t e8_max_steps() {
  if (const char* v = getenv("ZPAQ_AMD_E8_MAX_STEPS")) { const long long x = atoll(v); if (x > 0 && x < (long long)kE8MaxSteps) return (uint32_t)x; }
  return kE8MaxSteps;
}

// The filter's workspace, carved as the inverse's (engine_post.cpp une8_ws): the block table, the tiles' counts, the statuses,
// the scan's scratch
struct E8fWs { uint64_t o_cnt, o_st, o_tmp, bytes; size_t tmp_bytes; };
static E8fWs e8f_ws(size_t m, uint64_t ntiles) {
  E8fWs w;
  Carve cv;
  cv.take(m * sizeof(E8Block));
  w.o_cnt = cv.take(4 * (2 * ntiles + 1));
  w.o_st = cv.take(4 * m);
  w.tmp_bytes = une8_scan_bytes((uint32_t)ntiles);
  w.o_tmp = cv.take(w.tmp_bytes);
  w.bytes = cv.at + 256;
  return w;
}

// device/e8e9_forward_kernel.h over blocks that lie in d_buf, in place, wherever their offsets put them.  The caller has ensured
// e8f_ws(..).bytes of io_out and has nothing live in io_out or in the arena buffer: the workspace goes to the front of the one,
// the list of seeds and breaks -- sized from the two totals the host reads between the halves -- to the other.  held: what the
// call holds besides the arena buffer; arena_else: what that buffer has to hold afterwards anyway.  status[k] = 0: block k is
// filtered; 1: a lane gave it up, its bytes in d_buf are neither the input nor the output.  false + note: the device declines
// them all (the list beyond the budget, a failed launch) -- treat d_buf's copies as for status 1.
static bool engine_e8e9_forward(Engine& e, uint8_t* d_buf, const std::vector<E8Block>& blk, uint64_t ntiles, uint64_t held, uint64_t arena_else,
                                uint32_t max_steps, std::vector<uint32_t>& status, std::string& note) {
  const size_t m = blk.size();
  status.assign(m, 1u);
  if (!m) return true;
  const E8fWs w = e8f_ws(m, ntiles);
  uint8_t* const wb = (uint8_t*)e.io_out.p;
  uint32_t* const cnt = (uint32_t*)(wb + w.o_cnt);
  HIP_CHECK(hipMemcpyAsync(wb, blk.data(), m * sizeof(E8Block), hipMemcpyHostToDevice, e.stream));
  hipError_t rc = launch_e8f_mark(d_buf, (const E8Block*)wb, (uint32_t)m, (uint32_t)ntiles, cnt, (uint32_t*)(wb + w.o_st), wb + w.o_tmp, w.tmp_bytes, e.stream);
  if (launch_failed(rc, "device E8E9 filter failed: ", note)) return false;
  uint32_t nseeds = 0, nlist = 0;
  HIP_CHECK(hipMemcpyAsync(&nseeds, cnt + ntiles, 4, hipMemcpyDeviceToHost, e.stream));
  HIP_CHECK(hipMemcpyAsync(&nlist, cnt + 2 * ntiles, 4, hipMemcpyDeviceToHost, e.stream));
  HIP_CHECK(hipStreamSynchronize(e.stream));
  if (nseeds) {
    const uint64_t list_bytes = 4ull * nlist + 64;
    if (held + std::max(arena_else, list_bytes) + (1u << 20) > e.budget) { note = "the filter's list exceeds the device budget"; return false; }
    e.arena.ensure(list_bytes);
    rc = launch_e8f_walk(d_buf, (const E8Block*)wb, (uint32_t)m, (uint32_t)ntiles, cnt, (uint32_t*)e.arena.p, nseeds, max_steps, (uint32_t*)(wb + w.o_st), e.stream);
    if (launch_failed(rc, "device E8E9 filter failed: ", note)) return false;
  }
  HIP_CHECK(hipMemcpyAsync(status.data(), wb + w.o_st, 4 * m, hipMemcpyDeviceToHost, e.stream));
  HIP_CHECK(hipStreamSynchronize(e.stream));
  return true;
}

// The blocks of a batch that are to be filtered here (SortJob::e8): the list as the filter takes it, what it asks of io_out
struct E8Batch {
  std::vector<E8Block> blk;
  std::vector<size_t> who;
  uint64_t tiles = 0;
  void add(size_t i, uint64_t off, uint32_t n) {
    blk.push_back(E8Block{off, n, (uint32_t)tiles});
    who.push_back(i);
    tiles += e8_tiles(n);
  }
  uint64_t ws_bytes() const { return blk.empty() ? 0 : e8f_ws(blk.size(), tiles).bytes; }
};
static E8Batch e8_batch(const std::vector<SortJob>& jobs, const std::vector<HostItem>& items) {
  E8Batch b;
  for (size_t i = 0; i < jobs.size(); ++i) if (jobs[i].e8 && jobs[i].n) b.add(i, items[i].off, jobs[i].n);
  return b;
}
// ... and the filter over them, once their bytes lie in io_in where `b` says and before anything else reads them.  A block the
// device filtered comes down into the caller's buffer; one it declined is filtered there by the host and uploaded over the copy:
// either way both sides hold e8e9_forward's bytes when this returns, and *SortJob::e8 says who made them.  A throw before any
// download leaves every caller's buffer as it was (kE8Not) or filtered by the host (kE8Host).
static void filter_uploaded(Engine& e, const std::vector<SortJob>& jobs, const E8Batch& b, uint64_t held, uint64_t arena_else) {
  const size_t m = b.blk.size();
  if (!m) return;
  std::vector<uint32_t> st;
  std::string why;
  if (!engine_e8e9_forward(e, (uint8_t*)e.io_in.p, b.blk, b.tiles, held, arena_else, e8_max_steps(), st, why)) st.assign(m, 1u);
  for (size_t k = 0; k < m; ++k) {
    if (!st[k]) continue;
    const SortJob& j = jobs[b.who[k]];
    e8e9_forward(const_cast<U8*>(j.data), j.n);
    *j.e8 = kE8Host;
    HIP_CHECK(hipMemcpyAsync((uint8_t*)e.io_in.p + b.blk[k].off, j.data, j.n, hipMemcpyHostToDevice, e.stream));
  }
  for (size_t k = 0; k < m; ++k) {
    if (st[k]) continue;
    const SortJob& j = jobs[b.who[k]];
    *j.e8 = kE8InFlight;
    HIP_CHECK(hipMemcpyAsync(const_cast<U8*>(j.data), (const uint8_t*)e.io_in.p + b.blk[k].off, j.n, hipMemcpyDeviceToHost, e.stream));
  }
  HIP_CHECK(hipStreamSynchronize(e.stream));
  for (size_t k = 0; k < m; ++k) if (!st[k]) *jobs[b.who[k]].e8 = kE8Device;
}

bool engine_e8e9_device(U8* const* data, const U32* len, U32 n, U32 max_steps, int32_t* status, std::string& note) {
  for (U32 i = 0; i < n; ++i) status[i] = 1;
  E8Batch b;
  std::vector<HostItem> items(n);
  uint64_t total = 0;
  for (U32 i = 0; i < n; ++i) {
    items[i] = HostItem{data[i], len[i], total};
    b.add(i, total, len[i]);
    total += len[i];
  }
  if (n > 65535 || total >= (1ull << 31)) { note = "batch outside the device filter's range"; return false; }
  if (!n) return true;
  EngineCall call;
  Engine& e = call.e;
  const uint64_t in_bytes = align_up(total, 256) + 64, ws = b.ws_bytes();
  if (in_bytes + ws + (1u << 20) > e.budget) { note = "the batch exceeds the device budget"; return false; }
  e.io_in.ensure(in_bytes);
  e.io_out.ensure(ws);
  const auto staged = upload_staged(e, e.io_in.p, items, total, 0, total >= (1u << 20));
  std::vector<uint32_t> st;
  if (!engine_e8e9_forward(e, (uint8_t*)e.io_in.p, b.blk, b.tiles, in_bytes + ws, 0, max_steps ? max_steps : kE8MaxSteps, st, note)) return false;
  for (U32 i = 0; i < n; ++i)
    if (!st[i] && len[i]) HIP_CHECK(hipMemcpyAsync(data[i], (const uint8_t*)e.io_in.p + b.blk[i].off, len[i], hipMemcpyDeviceToHost, e.stream));
  HIP_CHECK(hipStreamSynchronize(e.stream));
  for (U32 i = 0; i < n; ++i) status[i] = st[i] ? 1 : 0;
  return true;
}

bool engine_suffix_arrays(const std::vector<std::pair<const U8*, U32>>& blocks, std::vector<std::vector<U32>>& sa, std::string& note) {
  const size_t n = blocks.size();
  sa.assign(n, std::vector<U32>());
  uint64_t total = 0;
  uint32_t max_len = 0;
  std::vector<HostItem> items(n);
  for (size_t i = 0; i < n; ++i) {
    items[i] = HostItem{blocks[i].first, blocks[i].second, total};
    total += blocks[i].second;
    max_len = std::max(max_len, blocks[i].second);
  }
  if (!total) return true;
  if (n > 65535 || max_len >= (1u << 24) || total >= (1ull << 31)) { note = "batch outside the device sorter's range"; return false; }
  EngineCall call;
  Engine& e = call.e;
  const size_t ws = sa_workspace_bytes(total, (uint32_t)n);
  const uint64_t in_bytes = align_up(total, 256);
  if (ws + in_bytes + 4 * total + (1u << 20) > e.budget) { note = "suffix sort workspace exceeds the device budget"; return false; }
  // inputs back to back in io_in, the arrays in io_out, the sorter's workspace in the arena buffer (idle between batches)
  e.io_in.ensure(in_bytes + 64);
  e.io_out.ensure(4 * total + 64);
  e.arena.ensure(ws);
  SaInputs in;
  upload_sa_inputs(e, items, total, in_bytes, in);
  uint32_t rounds = 0;
  const hipError_t rc = build_suffix_arrays(in.d_ptrs, in.d_off, (uint32_t)n, total, max_len, (uint32_t*)e.io_out.p, e.arena.p, e.arena.cap, e.stream, &rounds);
  if (launch_failed(rc, "device suffix sort failed: ", note)) return false;
  for (size_t i = 0; i < n; ++i) {
    sa[i].resize(blocks[i].second);
    if (blocks[i].second)
      HIP_CHECK(hipMemcpyAsync(sa[i].data(), (const uint32_t*)e.io_out.p + in.off[i], 4ull * blocks[i].second, hipMemcpyDeviceToHost, e.stream));
  }
  HIP_CHECK(hipStreamSynchronize(e.stream));
  note = "device, " + std::to_string(rounds) + " doubling rounds";
  return true;
}

// A block's entry in the table of the parse and code stages: where it lies, its kind, the coder's parameters, its token slots
// (tok_off for every block: the coder's item slots are found by it).  The parse stages add their search parameters.
static LzBlock lz_block(uint64_t off, uint32_t n, uint32_t kind, uint32_t min_match, uint32_t rb, uint64_t tok_off, uint32_t tok_cap) {
  LzBlock B;
  memset(&B, 0, sizeof(B));
  B.off = off;
  B.n = n;
  B.kind = kind;
  B.min_match = min_match;
  B.rb = rb;
  B.tok_off = tok_off;
  B.tok_cap = tok_cap;
  return B;
}

// Stages (c) and (d) of device/lz77_codes_kernel.h, behind launch_lz77_code_lengths on e.stream: the sizes and the error word come
// back, the streams are placed back to back (every start on a word) in the `room` bytes at d_out, emitted there and downloaded
// into dst[b] (null: not a block of kind 1 / 2).  Sizes first, then emission: a degenerate list can expand a block, no bound is
// guessed.  false + note: a list the host's coder refuses or an incomplete one (*refused says which), or no room.
static bool finish_lz77_codes(Engine& e, const std::vector<LzBlock>& blk, const uint8_t* d_in, uint64_t total, const LzBlock* d_blk, const LzTok* d_toks,
                              const uint32_t* d_counts, const LzCodes& c, uint64_t* d_ooff, uint8_t* d_out, uint64_t room,
                              const std::vector<std::vector<U8>*>& dst, std::string& note, uint32_t* refused) {
  const size_t n = blk.size();
  std::vector<uint32_t> sizes(n + 1);
  HIP_CHECK(hipMemcpyAsync(sizes.data(), c.sizes, 4 * (n + 1), hipMemcpyDeviceToHost, e.stream));
  HIP_CHECK(hipStreamSynchronize(e.stream));
  if (refused) *refused = sizes[n];
  if (sizes[n]) { note = (sizes[n] & kLzcErrList) ? "LZ77 token list refused by the coder's checks" : "LZ77 token list overflowed"; return false; }
  std::vector<uint64_t> ooff(n + 1, 0);
  for (size_t i = 0; i < n; ++i) ooff[i + 1] = ooff[i] + align_up(sizes[i], 4);
  if (ooff[n] > room) { note = "the coded streams do not fit the device's output buffer"; return false; }
  if (!ooff[n]) return true;
  HIP_CHECK(hipMemcpyAsync(d_ooff, ooff.data(), 8 * (n + 1), hipMemcpyHostToDevice, e.stream));
  HIP_CHECK(hipMemsetAsync(d_out, 0, ooff[n], e.stream));
  const hipError_t rc = launch_lz77_emit(d_in, d_blk, (uint32_t)n, total, d_toks, d_counts, c, d_ooff, d_out, e.stream);
  if (launch_failed(rc, "device LZ77 coder failed: ", note)) return false;
  for (size_t i = 0; i < n; ++i) {
    if (!dst[i]) continue;
    dst[i]->resize(sizes[i]);
    if (sizes[i]) HIP_CHECK(hipMemcpyAsync(dst[i]->data(), d_out + ooff[i], sizes[i], hipMemcpyDeviceToHost, e.stream));
  }
  HIP_CHECK(hipStreamSynchronize(e.stream));
  return true;
}
// codes == 2: does writing the codes here pay for this batch?  The sizes and the counts are on the device behind the walk.
static bool codes_pay(Engine& e, const std::vector<LzBlock>& blk, const LzCodes& c, const uint32_t* d_counts, uint64_t total) {
  const size_t n = blk.size();
  std::vector<uint32_t> sizes(n + 1), cnt(n);
  HIP_CHECK(hipMemcpyAsync(sizes.data(), c.sizes, 4 * (n + 1), hipMemcpyDeviceToHost, e.stream));
  HIP_CHECK(hipMemcpyAsync(cnt.data(), d_counts, 4 * n, hipMemcpyDeviceToHost, e.stream));
  HIP_CHECK(hipStreamSynchronize(e.stream));
  if (sizes[n]) return true;                         // (the error word: finish_lz77_codes reports it)
  uint64_t matches = 0, bytes = 0;
  for (size_t i = 0; i < n; ++i) { matches += cnt[i]; bytes += sizes[i]; }
  return lz_codes_pay(matches, bytes, total);
}
// the coder's share of a stage's buffer, behind what `cv` has carved so far: sizes + error word, the streams' places, lengths /
// offsets, scan scratch
struct CodesLayout { uint64_t o_sizes, o_ooff, o_pos, o_tmp, end; LzCodes c; };
static CodesLayout codes_layout(Carve cv, size_t n, uint64_t nslots) {
  CodesLayout L;
  L.c.nslots = nslots;
  L.c.tmp_bytes = lzc_scan_bytes(nslots);
  L.o_sizes = cv.take(4 * (n + 1));
  L.o_ooff = cv.take(8 * (n + 1));
  L.o_pos = cv.take(8 * (nslots + 1));
  L.o_tmp = cv.take(L.c.tmp_bytes);
  L.end = cv.at;
  return L;
}
static void codes_bind(CodesLayout& L, uint8_t* base) {
  L.c.pos = (uint64_t*)(base + L.o_pos);
  L.c.tmp = base + L.o_tmp;
  L.c.sizes = (uint32_t*)(base + L.o_sizes);
}

// Where a parse stage's arrays lie in io_out (`ob`), and the end of such a stage behind its launches: the blocks of kind 1 / 2
// come back as their finished streams -- codes 1, or 2 and that pays for this batch (lz_codes_pay); they take the place of the
// decisions at d_streams, which are dead behind the walk -- or as their lists of matches.  *coded says which.  false + note: a
// list overflowed, or the coder refused one.
struct ParseArrays { uint8_t* ob; uint64_t o_tok, o_cnt, o_blk; };
static bool parse_results(Engine& e, const std::vector<LzBlock>& blk, uint64_t total, int codes, const CodesLayout& cl, const ParseArrays& a, uint8_t* d_streams,
                          std::vector<SortOut>& out, std::string& note, bool* coded) {
  const size_t n = blk.size();
  const uint32_t* d_cnt = (const uint32_t*)(a.ob + a.o_cnt);
  if (codes == 2 && !codes_pay(e, blk, cl.c, d_cnt, total)) codes = 0;     // (the lists come back, as without the coder)
  *coded = codes != 0;
  if (codes) {
    std::vector<std::vector<U8>*> dst(n, nullptr);
    for (size_t i = 0; i < n; ++i)
      if (blk[i].kind == 1 || blk[i].kind == 2) { dst[i] = &out[i].codes; out[i].coded = true; }
    return finish_lz77_codes(e, blk, (const uint8_t*)e.io_in.p, total, (const LzBlock*)(a.ob + a.o_blk), (const LzTok*)(a.ob + a.o_tok), d_cnt, cl.c,
                             (uint64_t*)(a.ob + cl.o_ooff), d_streams, 16 * total, dst, note, nullptr);
  }
  std::vector<uint32_t> cnt(n);
  HIP_CHECK(hipMemcpyAsync(cnt.data(), d_cnt, 4 * n, hipMemcpyDeviceToHost, e.stream));
  HIP_CHECK(hipStreamSynchronize(e.stream));
  static_assert(sizeof(LzTok) == sizeof(LzToken) && sizeof(LzTok) == 16, "token layouts");
  for (size_t i = 0; i < n; ++i) {
    const LzBlock& B = blk[i];
    if (B.kind != 1 && B.kind != 2) continue;
    if (cnt[i] > B.tok_cap) { note = "LZ77 token list overflowed"; return false; }
    out[i].toks.resize(cnt[i]);
    if (cnt[i]) HIP_CHECK(hipMemcpyAsync(out[i].toks.data(), a.ob + a.o_tok + 16 * B.tok_off, 16ull * cnt[i], hipMemcpyDeviceToHost, e.stream));
  }
  HIP_CHECK(hipStreamSynchronize(e.stream));
  return true;
}

// The wide sorter for one block (device/sa_wide_kernel.h): the block up, the doubling rounds, then one of three ends.  Kind 3
// unless the caller wants the array: the BWT's last column straight from the ranks (n + 5 bytes come back).  Kind 1 / 2 with
// parse_codes >= 0: the parse in pieces (device/lz77_wide_kernel.h) and, as device_codes_mode says, LZBuffer's codes over a
// one-entry block table -- the list of matches or the stream comes back.  Else the array (4 n bytes; the host parses or
// transforms with it).  Everything the call holds on the device is summed against the budget before anything is launched.
// Blocks go one after another on the engine's stream.
static std::atomic<U32> g_last_wide_rounds{0};
U32 engine_last_wide_sort_rounds() { return g_last_wide_rounds.load(std::memory_order_relaxed); }
static std::atomic<U32> g_last_wide_pieces[4];
void engine_last_wide_parse_pieces(U32 out[4]) { for (int k = 0; k < 4; ++k) out[k] = g_last_wide_pieces[k].load(std::memory_order_relaxed); }

static uint32_t wide_piece() {
  U64 piece = kLzWidePiece;
  if (const char* v = getenv("ZPAQ_AMD_LZ_WIDE_PIECE")) { const long long x = atoll(v); if (x > 0) piece = (U64)x; }
  return lz_wide_piece_clamp(piece);
}
static bool wide_parse_in_range(const SortJob& j) {
  return (j.kind == 1 || j.kind == 2) && j.n < (1u << 31) && j.min_match >= 1 && j.lookahead <= 255 && j.checkbits >= 1 && j.checkbits <= 31 && j.rb <= 7;
}

// What a wide call holds on the device.  io_in: the block.  The arena buffer: the sorter's workspace (the ranks stay there for the
// search).  io_out: the array -- or the BWT's index word and column -- and, with the parse behind it, decisions (16 B per
// position), the final list, the pieces' slots, records and adoptions, the counts, the one-entry block table, the coder's arrays.
struct WidePlan {
  size_t ws = 0;
  uint64_t in_bytes = 0, sort_out = 0, parse_out = 0;
  LzWideParams W{};
  uint32_t tok_cap = 0;
  uint64_t o_res = 0, o_tok = 0, o_prov = 0, o_pieces = 0, o_adopt = 0, o_result = 0, o_blk = 0;
  CodesLayout cl;
  uint64_t held(bool parse) const { return ws + in_bytes + (parse ? parse_out : sort_out) + (1u << 20); }
};
static WidePlan wide_plan(const SortJob& job, bool bwt, uint32_t piece) {
  WidePlan P;
  const uint64_t n = job.n;
  P.ws = sa_wide_workspace_bytes(n);
  P.in_bytes = align_up(n, 256);
  P.sort_out = (bwt ? 256 + n + 1 : 4 * n) + 256;                      // (BWT: the index word in front of the column)
  P.parse_out = P.sort_out;
  if (bwt || !wide_parse_in_range(job)) return P;
  P.W.n = job.n;
  P.W.piece = piece;
  P.W.npieces = (uint32_t)((n + piece - 1) / piece);
  P.W.slot_cap = lz_wide_slot_cap(piece, job.min_match);
  P.tok_cap = job.n / job.min_match + 2;
  Carve cv;
  cv.take(4 * n);
  P.o_res = cv.take(16 * n);
  P.o_tok = cv.take(16ull * P.tok_cap);
  P.o_prov = cv.take(16ull * P.W.npieces * P.W.slot_cap);
  P.o_pieces = cv.take(sizeof(LzWidePiece) * (uint64_t)P.W.npieces);
  P.o_adopt = cv.take(sizeof(LzWideAdopt) * (uint64_t)P.W.npieces);
  P.o_result = cv.take(sizeof(LzWideResult));
  P.o_blk = cv.take(sizeof(LzBlock));
  P.cl = codes_layout(cv, 1, (uint64_t)P.tok_cap + 1);
  P.parse_out = P.cl.end + 256;
  return P;
}

void engine_wide_stage_bytes(const SortJob& job, U64 out[2]) {
  out[0] = out[1] = 0;
  if (!job.n) return;
  const WidePlan P = wide_plan(job, job.kind == 3, wide_piece());
  out[0] = P.held(false);
  out[1] = P.held(true);
}

// The parse behind the sort that has just run on e.stream (the array at the front of io_out, the ranks at d_rank).  false + note:
// a list overflowed, the coder refused it, a launch failed -- the array is still where it was.
static bool parse_wide(Engine& e, const SortJob& job, WidePlan& P, const uint32_t* d_rank, int codes, SortOut& out, std::string& note) {
  uint8_t* const ob = (uint8_t*)e.io_out.p;
  std::vector<LzBlock> blk(1, lz_block(0, job.n, job.kind, job.min_match, job.rb, 0, P.tok_cap));
  blk[0].lookahead = job.lookahead; blk[0].bucket = job.bucket; blk[0].checkbits = job.checkbits;
  HIP_CHECK(hipMemcpyAsync(ob + P.o_blk, blk.data(), sizeof(LzBlock), hipMemcpyHostToDevice, e.stream));
  HIP_CHECK(hipMemsetAsync(ob + P.o_result, 0, sizeof(LzWideResult), e.stream));
  if (codes) { codes_bind(P.cl, ob); HIP_CHECK(hipMemsetAsync(P.cl.c.sizes, 0, 4 * 2, e.stream)); }
  LzTok* const d_toks = (LzTok*)(ob + P.o_tok);
  LzWideResult* const d_result = (LzWideResult*)(ob + P.o_result);
  static_assert(offsetof(LzWideResult, count) == 0, "the coder reads the list's length as counts[0]");
  hipError_t rc = launch_lz77_wide((const uint8_t*)e.io_in.p, (const uint32_t*)ob, d_rank, (const LzBlock*)(ob + P.o_blk), P.W, P.tok_cap, ob + P.o_res,
                                   (LzTok*)(ob + P.o_prov), (LzWidePiece*)(ob + P.o_pieces), (LzWideAdopt*)(ob + P.o_adopt), d_toks, d_result, e.stream);
  if (rc == hipSuccess && codes) rc = launch_lz77_code_lengths((const LzBlock*)(ob + P.o_blk), 1, d_toks, (const uint32_t*)d_result, P.cl.c, e.stream);
  if (launch_failed(rc, "device wide parse failed: ", note)) return false;
  LzWideResult r;
  HIP_CHECK(hipMemcpyAsync(&r, d_result, sizeof r, hipMemcpyDeviceToHost, e.stream));
  HIP_CHECK(hipStreamSynchronize(e.stream));
  if (r.overflow || r.count > P.tok_cap || r.pieces != P.W.npieces) { note = "LZ77 token list overflowed"; return false; }
  std::vector<SortOut> outs(1);
  bool coded = false;
  if (!parse_results(e, blk, job.n, codes, P.cl, ParseArrays{ob, P.o_tok, P.o_result, P.o_blk}, ob + P.o_res, outs, note, &coded)) return false;
  out = std::move(outs[0]);
  out.parsed = true;
  g_last_wide_pieces[0].store(r.pieces, std::memory_order_relaxed);
  for (int k = 0; k < 3; ++k) g_last_wide_pieces[1 + k].store(r.how[k], std::memory_order_relaxed);
  return true;
}

bool engine_sort_wide(const SortJob& job, SortOut& out, std::string& note, bool want_sa, int parse_codes, bool parse_or_nothing) {
  out = SortOut();
  const uint64_t n = job.n;
  if (!n) return true;
  if (n >= (1ull << 31)) { note = "block outside the wide sorter's range"; return false; }
  if (job.kind > 3) { note = "unknown pre-processor kind"; return false; }
  const bool bwt = job.kind == 3 && !want_sa;
  bool parse = !want_sa && parse_codes >= 0 && (job.kind == 1 || job.kind == 2);
  std::string why;                                              // why the parse did not run here although it was asked for
  if (parse && !wide_parse_in_range(job)) { parse = false; why = "LZ77 parameters outside the device parser's range"; }
  EngineCall call;
  Engine& e = call.e;
  WidePlan P = wide_plan(job, bwt, wide_piece());
  if (parse && P.held(true) > e.budget) { parse = false; why = "sort + parse workspace exceeds the device budget"; }
  if (parse_or_nothing && !parse) { note = why.empty() ? "the block is not one the device parses" : why; return false; }   // (nothing was launched)
  if (P.held(false) > e.budget) { note = "suffix sort workspace exceeds the device budget"; return false; }
  E8Batch e8;
  if (job.e8) e8.add(0, 0, job.n);
  const uint64_t out_bytes = std::max<uint64_t>(parse ? P.parse_out : P.sort_out, e8.ws_bytes());
  e.io_in.ensure(P.in_bytes + 64);
  e.io_out.ensure(out_bytes);
  e.arena.ensure(P.ws);
  HIP_CHECK(hipMemcpyAsync(e.io_in.p, job.data, n, hipMemcpyHostToDevice, e.stream));
  filter_uploaded(e, std::vector<SortJob>(1, job), e8, P.in_bytes + out_bytes, P.ws);
  uint8_t* const ob = (uint8_t*)e.io_out.p;
  uint32_t rounds = 0;
  const uint32_t* d_rank = nullptr;
  hipError_t rc = build_suffix_array_wide((const uint8_t*)e.io_in.p, (uint32_t)n, bwt ? nullptr : (uint32_t*)ob, e.arena.p, e.arena.cap, e.stream, &rounds, &d_rank);
  if (rc == hipSuccess && bwt) rc = launch_bwt_wide((const uint8_t*)e.io_in.p, d_rank, (uint32_t)n, ob + 256, (uint32_t*)ob, e.stream);
  if (launch_failed(rc, "device wide suffix sort failed: ", note)) return false;
  g_last_wide_rounds.store(rounds, std::memory_order_relaxed);
  note = "device (wide), " + std::to_string(rounds) + " doubling rounds";
  if (parse) {
    if (parse_wide(e, job, P, d_rank, parse_codes, out, why)) { note += out.coded ? ", parsed and coded there" : ", parsed there"; return true; }
    out = SortOut();                                            // (the array is still at the front of io_out: the host parses with it)
  }
  if (!why.empty()) note += "; " + why;
  if (bwt) {
    uint32_t idx = 0;
    out.bwt.resize((size_t)n + 5);
    HIP_CHECK(hipMemcpyAsync(out.bwt.data(), ob + 256, (size_t)n + 1, hipMemcpyDeviceToHost, e.stream));
    HIP_CHECK(hipMemcpyAsync(&idx, ob, 4, hipMemcpyDeviceToHost, e.stream));
    HIP_CHECK(hipStreamSynchronize(e.stream));
    for (int k = 0; k < 4; ++k) { out.bwt[(size_t)n + 1 + k] = (U8)idx; idx >>= 8; }
  } else {
    out.sa.resize((size_t)n);
    HIP_CHECK(hipMemcpyAsync(out.sa.data(), ob, 4 * n, hipMemcpyDeviceToHost, e.stream));
    HIP_CHECK(hipStreamSynchronize(e.stream));
  }
  return true;
}

bool engine_sort_preprocess(const std::vector<SortJob>& jobs, std::vector<SortOut>& out, std::string& note, int codes) {
  const size_t n = jobs.size();
  out.assign(n, SortOut());
  uint64_t total = 0, ntok = 0, bwt_bytes = 0;
  uint32_t max_len = 0;
  bool any_lz = false, any_bwt = false;
  std::vector<LzBlock> blk(n);
  std::vector<HostItem> items(n);
  for (size_t i = 0; i < n; ++i) {
    const SortJob& j = jobs[i];
    LzBlock& B = blk[i] = lz_block(total, j.n, j.n ? j.kind : 0u, j.min_match, j.rb, ntok, 0);
    B.lookahead = j.lookahead; B.bucket = j.bucket; B.checkbits = j.checkbits;
    if (B.kind == 1 || B.kind == 2) {
      if (j.min_match < 1 || j.lookahead > 255 || j.checkbits < 1 || j.checkbits > 31) { note = "LZ77 parameters outside the device parser's range"; return false; }
      B.tok_cap = j.n / j.min_match + 2;
      ntok += B.tok_cap;
      any_lz = true;
    } else if (B.kind == 3) {
      any_bwt = true;
    } else if (B.kind != 0) { note = "unknown pre-processor kind"; return false; }
    items[i] = HostItem{j.data, j.n, total};
    total += j.n;
    max_len = std::max(max_len, j.n);
  }
  if (!total) return true;
  bwt_bytes = any_bwt ? total + n : 0;
  if (n > 65535 || max_len >= (1u << 24) || total >= (1ull << 31)) { note = "batch outside the device sorter's range"; return false; }
  EngineCall call;
  Engine& e = call.e;
  const size_t ws = sa_workspace_bytes(total, (uint32_t)n);
  const uint64_t in_bytes = align_up(total, 256);
  // io_out: the arrays, then decisions (16 B per element), tokens, BWT bytes, counts and indices, the block table
  Carve cv;
  cv.take(4 * total);
  const uint64_t o_res = cv.take(any_lz ? 16 * total : 0);
  const uint64_t o_tok = cv.take(16 * ntok, 1);
  const uint64_t o_bwt = cv.take(bwt_bytes, 1);
  const uint64_t o_cnt = cv.take(4 * n);
  const uint64_t o_idx = cv.take(4 * n, 1);
  const uint64_t o_blk = cv.take(n * sizeof(LzBlock));
  if (!any_lz) codes = 0;
  // ... and the coder's arrays (device/lz77_codes_kernel.h); the streams themselves take the place of the decisions, which are
  // dead behind the walk
  CodesLayout cl = codes_layout(cv, n, ntok + n);
  const E8Batch e8 = e8_batch(jobs, items);
  const uint64_t out_bytes = std::max<uint64_t>((codes ? cl.end : cv.at) + 256, e8.ws_bytes());
  if (ws + in_bytes + out_bytes + (1u << 20) > e.budget) { note = "sort + parse workspace exceeds the device budget"; return false; }
  e.io_in.ensure(in_bytes + 64);
  e.io_out.ensure(out_bytes);
  e.arena.ensure(ws);
  SaInputs in;
  upload_sa_inputs(e, items, total, in_bytes, in);
  filter_uploaded(e, jobs, e8, in_bytes + out_bytes, ws);
  uint8_t* const ob = (uint8_t*)e.io_out.p;
  HIP_CHECK(hipMemcpyAsync(ob + o_blk, blk.data(), n * sizeof(LzBlock), hipMemcpyHostToDevice, e.stream));
  HIP_CHECK(hipMemsetAsync(ob + o_cnt, 0, 8 * n, e.stream));
  if (codes) { codes_bind(cl, ob); HIP_CHECK(hipMemsetAsync(cl.c.sizes, 0, 4 * (n + 1), e.stream)); }
  uint32_t rounds = 0;
  SaSideArrays side;
  hipError_t rc = build_suffix_arrays(in.d_ptrs, in.d_off, (uint32_t)n, total, max_len, (uint32_t*)ob, e.arena.p, e.arena.cap, e.stream, &rounds, &side);
  if (rc == hipSuccess)
    rc = launch_sort_preprocessors((const uint8_t*)e.io_in.p, (const uint32_t*)ob, side, (const LzBlock*)(ob + o_blk), (uint32_t)n, total, any_lz, any_bwt,
                                   ob + o_res, (LzTok*)(ob + o_tok), (uint32_t*)(ob + o_cnt), ob + o_bwt, (uint32_t*)(ob + o_idx), e.stream,
                                   codes ? &cl.c : nullptr);
  if (launch_failed(rc, "device sort / parse failed: ", note)) return false;
  bool coded = false;
  if (any_lz && !parse_results(e, blk, total, codes, cl, ParseArrays{ob, o_tok, o_cnt, o_blk}, ob + o_res, out, note, &coded)) return false;
  if (any_bwt) {
    std::vector<uint32_t> idx(n);
    HIP_CHECK(hipMemcpyAsync(idx.data(), ob + o_idx, 4 * n, hipMemcpyDeviceToHost, e.stream));
    HIP_CHECK(hipStreamSynchronize(e.stream));
    for (size_t i = 0; i < n; ++i) {
      const LzBlock& B = blk[i];
      if (B.kind != 3) continue;
      out[i].bwt.resize((size_t)B.n + 5);
      HIP_CHECK(hipMemcpyAsync(out[i].bwt.data(), ob + o_bwt + B.off + i, (size_t)B.n + 1, hipMemcpyDeviceToHost, e.stream));
      for (int k = 0; k < 4; ++k) { out[i].bwt[(size_t)B.n + 1 + k] = (U8)idx[i]; idx[i] >>= 8; }
    }
    HIP_CHECK(hipStreamSynchronize(e.stream));
  }
  note = "device, " + std::to_string(rounds) + " doubling rounds";
  return true;
}

bool engine_hash_preprocess(const std::vector<SortJob>& jobs, std::vector<SortOut>& out, std::string& note, int codes) {
  const size_t n = jobs.size();
  out.assign(n, SortOut());
  uint64_t total = 0, ntok = 0, nkeys = 0, nidx = 0;
  std::vector<LzBlock> blk(n);
  std::vector<HostItem> items(n);
  for (size_t i = 0; i < n; ++i) {
    const SortJob& j = jobs[i];
    if (!hash_job_in_range(j)) { note = "LZ77 parameters or block size outside the device hash parser's range"; return false; }
    LzBlock& B = blk[i] = lz_block(total, j.n, j.n ? j.kind : 0u, j.min_match, j.rb, ntok, j.n / j.min_match + 2);
    B.lookahead = j.lookahead; B.bucket = j.bucket; B.checkbits = j.checkbits;
    B.min_match2 = j.min_match2; B.ht_bits = j.ht_bits;
    ntok += B.tok_cap;
    lz_hash_plan(B, nkeys, nidx);
    items[i] = HostItem{j.data, j.n, total};
    total += j.n;
  }
  if (!total) return true;
  if (n > 65535 || total >= (1ull << 31)) { note = "batch outside the device hash parser's range"; return false; }
  EngineCall call;
  Engine& e = call.e;
  const size_t ws = lzh_workspace_bytes(total, nkeys, nidx);
  const uint64_t in_bytes = align_up(total, 256);
  // io_out: decisions (16 B per element), tokens, counts, the block table
  Carve cv;
  cv.take(16 * total);
  const uint64_t o_tok = cv.take(16 * ntok, 1);
  const uint64_t o_cnt = cv.take(4 * n);
  const uint64_t o_blk = cv.take(n * sizeof(LzBlock));
  // ... and the coder's arrays; the streams take the place of the decisions (device/lz77_codes_kernel.h)
  CodesLayout cl = codes_layout(cv, n, ntok + n);
  const E8Batch e8 = e8_batch(jobs, items);
  const uint64_t out_bytes = std::max<uint64_t>((codes ? cl.end : cv.at) + 256, e8.ws_bytes());
  if (ws + in_bytes + out_bytes + (1u << 20) > e.budget) { note = "hash parse workspace exceeds the device budget"; return false; }
  e.io_in.ensure(in_bytes + 64);
  e.io_out.ensure(out_bytes);
  e.arena.ensure(ws);
  const auto staged = upload_staged(e, e.io_in.p, items, total, 0, in_bytes >= (1u << 20));
  filter_uploaded(e, jobs, e8, in_bytes + out_bytes, ws);
  uint8_t* const ob = (uint8_t*)e.io_out.p;
  HIP_CHECK(hipMemcpyAsync(ob + o_blk, blk.data(), n * sizeof(LzBlock), hipMemcpyHostToDevice, e.stream));
  HIP_CHECK(hipMemsetAsync(ob + o_cnt, 0, 4 * n, e.stream));
  if (codes) { codes_bind(cl, ob); HIP_CHECK(hipMemsetAsync(cl.c.sizes, 0, 4 * (n + 1), e.stream)); }
  const hipError_t rc = launch_hash_parse((const uint8_t*)e.io_in.p, (const LzBlock*)(ob + o_blk), (uint32_t)n, total, nkeys, nidx, e.arena.p, e.arena.cap,
                                          ob, (LzTok*)(ob + o_tok), (uint32_t*)(ob + o_cnt), e.stream, codes ? &cl.c : nullptr);
  if (launch_failed(rc, "device hash parse failed: ", note)) return false;
  bool coded = false;
  if (!parse_results(e, blk, total, codes, cl, ParseArrays{ob, o_tok, o_cnt, o_blk}, ob, out, note, &coded)) return false;
  note = "device, " + std::to_string(nkeys) + (coded ? " keys, coded there" : " keys");
  return true;
}

int engine_lz77_codes(const std::vector<CodeJob>& jobs, std::vector<std::vector<U8>>& out, std::string& note) {
  const size_t n = jobs.size();
  out.assign(n, std::vector<U8>());
  if (!n) return 1;
  uint64_t total = 0, ntok = 0;
  std::vector<LzBlock> blk(n);
  std::vector<HostItem> items(n);
  std::vector<uint32_t> cnt(n);
  bool in_range = n <= 65535;
  for (size_t i = 0; i < n && in_range; ++i) {
    const CodeJob& j = jobs[i];
    in_range = j.n < (1u << 24) && (j.kind == 1 || j.kind == 2) && j.min_match >= 1 && j.min_match <= 255 && j.rb <= 7 && j.ntok <= (size_t)j.n + 1;
    cnt[i] = (uint32_t)j.ntok;
    blk[i] = lz_block(total, j.n, j.kind, j.min_match, j.rb, ntok, cnt[i]);      // (the kind also for an empty block: a list over it must be refused)
    items[i] = HostItem{j.data, j.n, total};
    ntok += j.ntok;
    total += j.n;
  }
  // (a list of more than n + 1 tokens cannot be in order: positions rise strictly -- but saying so is the kernel's job; such a
  // list is merely outside what the buffers are sized for)
  if (!in_range || total >= (1ull << 31)) { note = "batch outside the device coder's range"; return -1; }
  EngineCall call;
  Engine& e = call.e;
  // the arena buffer (idle between batches): tokens, counts, the block table, the coder's arrays; inputs in io_in, streams in io_out
  Carve cv;
  cv.take(16 * ntok);
  const uint64_t o_cnt = cv.take(4 * n);
  const uint64_t o_blk = cv.take(n * sizeof(LzBlock));
  CodesLayout cl = codes_layout(cv, n, ntok + n);
  const uint64_t ws = cl.end + 256, in_bytes = align_up(total, 256);
  if (ws + in_bytes + (1u << 20) > e.budget) { note = "coder workspace exceeds the device budget"; return -1; }
  e.io_in.ensure(in_bytes + 64);
  e.arena.ensure(ws);
  uint8_t* const ab = (uint8_t*)e.arena.p;
  codes_bind(cl, ab);
  std::vector<LzToken> toks(ntok + 1);
  for (size_t i = 0; i < n; ++i)
    if (jobs[i].ntok) memcpy(toks.data() + blk[i].tok_off, jobs[i].toks, 16 * jobs[i].ntok);
  static_assert(sizeof(LzTok) == sizeof(LzToken) && sizeof(LzTok) == 16, "token layouts");
  const auto staged = upload_staged(e, e.io_in.p, items, total, 0, false);
  if (ntok) HIP_CHECK(hipMemcpyAsync(ab, toks.data(), 16 * ntok, hipMemcpyHostToDevice, e.stream));
  HIP_CHECK(hipMemcpyAsync(ab + o_cnt, cnt.data(), 4 * n, hipMemcpyHostToDevice, e.stream));
  HIP_CHECK(hipMemcpyAsync(ab + o_blk, blk.data(), n * sizeof(LzBlock), hipMemcpyHostToDevice, e.stream));
  HIP_CHECK(hipMemsetAsync(cl.c.sizes, 0, 4 * (n + 1), e.stream));
  const hipError_t rc = launch_lz77_code_lengths((const LzBlock*)(ab + o_blk), (uint32_t)n, (const LzTok*)ab, (const uint32_t*)(ab + o_cnt), cl.c, e.stream);
  if (launch_failed(rc, "device LZ77 coder failed: ", note)) return -1;
  // sizes first: the streams' room is claimed once they are known
  std::vector<uint32_t> sizes(n + 1);
  HIP_CHECK(hipMemcpyAsync(sizes.data(), cl.c.sizes, 4 * (n + 1), hipMemcpyDeviceToHost, e.stream));
  HIP_CHECK(hipStreamSynchronize(e.stream));
  if (sizes[n]) { note = "LZ77 token list refused by the coder's checks"; return 0; }
  uint64_t room = 0;
  for (size_t i = 0; i < n; ++i) room += align_up(sizes[i], 4);
  if (ws + in_bytes + room + (1u << 20) > e.budget) { note = "the coded streams exceed the device budget"; return -1; }
  e.io_out.ensure(room + 64);
  std::vector<std::vector<U8>*> dst(n);
  for (size_t i = 0; i < n; ++i) dst[i] = &out[i];
  uint32_t refused = 0;
  if (!finish_lz77_codes(e, blk, (const uint8_t*)e.io_in.p, total, (const LzBlock*)(ab + o_blk), (const LzTok*)ab, (const uint32_t*)(ab + o_cnt), cl.c,
                         (uint64_t*)(ab + cl.o_ooff), (uint8_t*)e.io_out.p, room, dst, note, &refused))
    return refused ? 0 : -1;
  return 1;
}

// device/fragment_kernel.h for a batch of host files: one upload, round 0 (every piece from its own start), the stitch rounds
// (engine.hpp), one SHA-1 job per final fragment.  The records of a launch come back in runs of neighbouring lists.
static std::atomic<U32> g_last_fragment_rounds{0};
U32 engine_last_fragment_rounds() { return g_last_fragment_rounds.load(std::memory_order_relaxed); }

int engine_fragment(const U8* const* in, const U64* len, U32 n, const FragLimits& lim, std::vector<std::vector<Fragment>>& out, std::string& note) {
  out.assign(n, std::vector<Fragment>());
  g_last_fragment_rounds.store(0, std::memory_order_relaxed);
  if (!n) return 1;
  U64 piece = std::max<U64>(kFragPiece, 64ull * lim.min_frag);    // (walks re-join after a few fragments: keep that a fraction of a piece)
  if (const char* v = getenv("ZPAQ_AMD_FRAG_PIECE")) { const long long x = atoll(v); if (x > 0) piece = (U64)x; }
  piece = std::min<U64>(std::max<U64>(piece, 64), 1u << 30);
  if (n > 65535) { note = "more than 65 535 files in one batch"; return -1; }
  if (!lim.min_frag || lim.max_frag < lim.min_frag) { note = "fragment limits out of range"; return -1; }
  std::vector<U64> off(n);
  U64 bytes = 0;
  for (U32 f = 0; f < n; ++f) {
    off[f] = bytes;
    if (len[f] > (1ull << 31)) { note = "more than 2 GiB of input in one batch"; return -1; }
    bytes += align_up(len[f], 64);
  }
  if (bytes > (1ull << 31)) { note = "more than 2 GiB of input in one batch"; return -1; }
  FragPlan pl;
  if (!frag_plan(len, n, piece, lim.min_frag, pl)) { note = "the record lists exceed the device budget"; return -1; }
  const size_t m = pl.pc.size();
  const U64 nrec = pl.nrec;
  const bool pieces = pl.pieces;                    // fix-ups write into a second set of lists
  const U64 rec_bytes = nrec * sizeof(FragRec) * (pieces ? 2u : 1u);
  EngineCall call;
  Engine& e = call.e;
  if (bytes + rec_bytes + m * (sizeof(FragJob) + sizeof(FragResult)) + (1u << 20) > e.budget) { note = "the files and the record lists exceed the device budget"; return -1; }
  e.io_in.ensure(bytes + 64);
  e.io_out.ensure(rec_bytes + 64);
  e.jobs.ensure(m * sizeof(FragJob));
  e.results.ensure(m * sizeof(FragResult));
  uint8_t* const ib = (uint8_t*)e.io_in.p;
  FragRec* const recs = (FragRec*)e.io_out.p;
  // the upload: a large file goes as it lies, runs of small ones through one staging buffer
  const U64 kDirect = 1u << 20;
  U64 small = 0;
  for (U32 f = 0; f < n; ++f) if (len[f] < kDirect) small += align_up(len[f], 64);
  std::unique_ptr<uint8_t[]> stage(new uint8_t[small + 64]);
  U64 at = 0;
  for (U32 f = 0; f < n;) {
    if (len[f] >= kDirect) { HIP_CHECK(hipMemcpyAsync(ib + off[f], in[f], len[f], hipMemcpyHostToDevice, e.stream)); ++f; continue; }
    const U32 f0 = f;
    const U64 at0 = at;
    for (; f < n && len[f] < kDirect; ++f) {
      if (len[f]) memcpy(stage.get() + at, in[f], len[f]);
      at += align_up(len[f], 64);
    }
    if (at > at0) HIP_CHECK(hipMemcpyAsync(ib + off[f0], stage.get() + at0, at - at0, hipMemcpyHostToDevice, e.stream));
  }
  FragParams P;
  P.min_frag = lim.min_frag; P.max_frag = lim.max_frag; P.thresh = lim.thresh;
  // one launch: the jobs up, the walk, how each ended and its records down (the jobs' lists ascend in the record array)
  auto run = [&](const std::vector<FragJob>& jb, std::vector<FragResult>& rs, std::vector<std::vector<FragRec>>& lists) -> bool {
    const size_t q = jb.size();
    rs.resize(q);
    lists.assign(q, std::vector<FragRec>());
    HIP_CHECK(hipMemcpyAsync(e.jobs.p, jb.data(), q * sizeof(FragJob), hipMemcpyHostToDevice, e.stream));
    const hipError_t rc = launch_frag_walk(ib, (const FragJob*)e.jobs.p, (uint32_t)q, P, recs, (FragResult*)e.results.p, e.stream);
    if (launch_failed(rc, "device fragment walk failed: ", note)) return false;
    HIP_CHECK(hipMemcpyAsync(rs.data(), e.results.p, q * sizeof(FragResult), hipMemcpyDeviceToHost, e.stream));
    HIP_CHECK(hipStreamSynchronize(e.stream));
    if (!frag_results_ok(jb, rs)) { note = "device fragment walk: a record list overflowed"; return false; }
    std::vector<FragRec> tmp;
    for (size_t i = 0; i < q;) {
      size_t j = i;
      const U64 a = jb[i].rec_off;
      U64 b = a + rs[i].count;
      while (j + 1 < q && jb[j + 1].rec_off - b <= 256u && jb[j + 1].rec_off + rs[j + 1].count - a <= (1u << 16)) { ++j; b = (U64)jb[j].rec_off + rs[j].count; }
      tmp.resize((size_t)(b - a));
      HIP_CHECK(hipMemcpyAsync(tmp.data(), recs + a, (size_t)(b - a) * sizeof(FragRec), hipMemcpyDeviceToHost, e.stream));
      HIP_CHECK(hipStreamSynchronize(e.stream));
      for (size_t k = i; k <= j; ++k) lists[k].assign(tmp.begin() + (jb[k].rec_off - a), tmp.begin() + (jb[k].rec_off - a) + rs[k].count);
      i = j + 1;
    }
    return true;
  };
  std::vector<std::vector<FragRec>> fin;
  U32 rounds = 0;
  if (!frag_stitch(pl, off.data(), len, n, piece, run, fin, rounds, note)) return -1;
  // one SHA-1 job per fragment
  U64 total = 0;
  for (U32 f = 0; f < n; ++f) total += fin[f].size();
  if (total >= (1ull << 31)) { note = "too many fragments"; return -1; }
  std::vector<Sha1Job> sj((size_t)total);
  size_t s = 0;
  for (U32 f = 0; f < n; ++f) {
    uint32_t from = 0;
    out[f].resize(fin[f].size());
    for (size_t k = 0; k < fin[f].size(); ++k) {
      const FragRec& r = fin[f][k];
      Fragment& o = out[f][k];
      o.size = r.end - from;
      o.hits = r.hits;
      memcpy(o.o1, r.o1, 256);
      sj[s] = Sha1Job{ib + off[f] + from, o.size, (uint32_t)s};
      ++s;
      from = r.end;
    }
  }
  std::vector<uint8_t> dig((size_t)total * 20);
  sha1_round_trip(e, sj, dig.data());
  s = 0;
  for (U32 f = 0; f < n; ++f) for (Fragment& o : out[f]) { memcpy(o.sha1, dig.data() + 20 * s, 20); ++s; }
  g_last_fragment_rounds.store(rounds, std::memory_order_relaxed);
  return 1;
}

}  // namespace zpq
