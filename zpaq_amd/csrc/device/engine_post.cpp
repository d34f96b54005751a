// The engine's batch stages of the decompression side: the archive's own PCOMP program a lane per segment, and the decoders of the
// standard methods' streams -- LZ77, BWT, and either (or nothing) behind the inverse E8E9 filter.  Each takes the engine for one
// call (EngineCall), sums what its batch holds on the device against the engine's budget, stages its inputs, launches, and
// delivers or declines.
#include <algorithm>

#include "engine_internal.hpp"
#include "kernels.h"
#include "sa_kernels.h"
#include "spec_loader.hpp"

namespace zpq {

bool engine_pcomp(const U8* code, size_t codelen, int ph, int pm, std::vector<PcompSeg>& segs, std::string& note, bool* handed_back) {
  if (handed_back) *handed_back = false;
  if (segs.empty()) return true;
  EngineCall call;
  Engine& e = call.e;
  PcompKernel* k = pcomp_kernel_for(code, codelen, ph, pm, note);
  if (!k) return false;
  if (handed_back) *handed_back = true;          // (every false from here on)
  const size_t n = segs.size();
  const uint64_t mbytes = align_up(1ull << pm, 256), hbytes = align_up(4ull << ph, 256);
  std::vector<uint64_t> cap(n);
  for (size_t i = 0; i < n; ++i) cap[i] = (segs[i].hint ? segs[i].hint : 8ull * segs[i].in_len) + 65536;
  for (int attempt = 0; attempt < 2; ++attempt) {
    uint64_t in_bytes = 0, out_bytes = 0;
    for (size_t i = 0; i < n; ++i) {
      if (cap[i] > 0xFFFFFFF0ull) { note = "segment output beyond the device kernel's 32-bit range"; return false; }   // the host runs it (the size hint is a comment the reference ignores)
      in_bytes += align_up(segs[i].in_len, 64);
      out_bytes += align_up(cap[i], 64);
    }
    const uint64_t work = (uint64_t)n * (mbytes + hbytes + 1024);
    if (in_bytes + out_bytes + work > e.budget) { note = "post-processor state exceeds the device budget"; return false; }
    e.io_in.ensure(in_bytes + 64);
    e.io_out.ensure(out_bytes + 64);
    e.arena.ensure(work);
    e.jobs.ensure(n * sizeof(PcompJob));
    e.results.ensure(n * 8);
    std::vector<HostItem> items(n);
    std::vector<PcompJob> jobs(n);
    std::vector<uint64_t> ooff(n);
    uint64_t io = 0, oo = 0;
    for (size_t i = 0; i < n; ++i) {
      items[i] = HostItem{segs[i].in, segs[i].in_len, io};
      PcompJob& j = jobs[i];
      j.in = (const uint8_t*)e.io_in.p + io;
      j.out = (uint8_t*)e.io_out.p + oo;
      uint8_t* w = (uint8_t*)e.arena.p + (uint64_t)i * (mbytes + hbytes + 1024);
      j.M = w;
      j.H = (uint32_t*)(w + mbytes);
      j.R = (uint32_t*)(w + mbytes + hbytes);
      j.in_len = segs[i].in_len;
      j.out_cap = (uint32_t)cap[i];
      j.result = (uint32_t*)e.results.p + 2 * i;
      ooff[i] = oo;
      io += align_up(segs[i].in_len, 64);
      oo += align_up(cap[i], 64);
    }
    HIP_CHECK(hipMemsetAsync(e.arena.p, 0, work, e.stream));
    const auto staged = upload_staged(e, e.io_in.p, items, in_bytes, 64, false);
    HIP_CHECK(hipMemcpyAsync(e.jobs.p, jobs.data(), n * sizeof(PcompJob), hipMemcpyHostToDevice, e.stream));
    const PcompJob* d_jobs = (const PcompJob*)e.jobs.p;
    unsigned nn = (unsigned)n;
    void* args[2] = {(void*)&d_jobs, (void*)&nn};
    HIP_CHECK(hipModuleLaunchKernel(k->fn, (unsigned)((n + 63) / 64), 1, 1, 64, 1, 1, 0, e.stream, args, nullptr));
    std::vector<uint32_t> res(2 * n);
    HIP_CHECK(hipMemcpyAsync(res.data(), e.results.p, n * 8, hipMemcpyDeviceToHost, e.stream));
    HIP_CHECK(hipStreamSynchronize(e.stream));
    bool again = false;
    for (size_t i = 0; i < n; ++i) {
      // a device status is not a verdict: the translated program has a fixed budget of backward jumps, so the host
      // post-processor (which owns the ZPAQL-error decision, like the reference's) runs these segments again
      if (res[2 * i + 1]) { note = "device post-processor stopped (status " + std::to_string(res[2 * i + 1]) + "): host fallback"; return false; }
      if (res[2 * i] > cap[i]) { cap[i] = res[2 * i]; again = true; }
    }
    if (again && attempt == 0) continue;
    for (size_t i = 0; i < n; ++i) {
      segs[i].out->resize(res[2 * i]);
      if (res[2 * i])
        HIP_CHECK(hipMemcpyAsync(segs[i].out->data(), (const uint8_t*)e.io_out.p + ooff[i], res[2 * i], hipMemcpyDeviceToHost, e.stream));
    }
    HIP_CHECK(hipStreamSynchronize(e.stream));
    return true;
  }
  return false;
}

// The download of a decoded block (`len` bytes at `off` of io_out): into the job's vector, resized, when it has one, else into
// its buffer
static void deliver(Engine& e, StreamJob& j, uint64_t off, uint64_t len) {
  if (j.vec) j.vec->resize(len);
  uint8_t* dst = j.vec ? j.vec->data() : j.out;
  if (len) HIP_CHECK(hipMemcpyAsync(dst, (const uint8_t*)e.io_out.p + off, len, hipMemcpyDeviceToHost, e.stream));
}
// the device declines the batch behind the point where sizes were reported: none stays (-1 + note)
static int declined(std::vector<StreamJob>& jobs) {
  for (StreamJob& j : jobs) j.out_len = 0;
  return -1;
}

// device/e8e9_kernel.h over blocks that lie in io_out, in place.  The caller placed them (offsets multiples of 16, the rooms rounded
// up) and ensured une8_ws(..).bytes of io_out at ws_off (a multiple of 256) for the first half: the block table, the tiles' counts,
// the statuses, the scan's scratch.  The list of seeds and breaks is sized from the two totals the host reads between the halves
// and goes to io_in, whose content the caller needs no longer; `held` = what the batch holds besides it.  status[k] = 0: block k
// is filtered; 1: a lane gave it up, its bytes are to be dropped.  false + note: nothing is to be delivered.
struct E8Ws { uint64_t o_cnt, o_st, o_tmp, bytes; size_t tmp_bytes; };
static E8Ws une8_ws(size_t m, uint64_t ntiles) {
  E8Ws w;
  Carve cv;
  cv.take(m * sizeof(E8Block));
  w.o_cnt = cv.take(4 * (2 * ntiles + 1));
  w.o_st = cv.take(4 * m);
  w.tmp_bytes = une8_scan_bytes((uint32_t)ntiles);
  w.o_tmp = cv.take(w.tmp_bytes);
  w.bytes = cv.at + 256;
  return w;
}
static bool une8_run(Engine& e, uint64_t ws_off, const std::vector<E8Block>& blk, uint64_t ntiles, uint64_t held, std::vector<uint32_t>& status,
                     std::string& note) {
  const size_t m = blk.size();
  status.assign(m, 1u);
  if (!m) return true;
  const E8Ws w = une8_ws(m, ntiles);
  uint8_t* const ob = (uint8_t*)e.io_out.p;
  uint8_t* const wb = ob + ws_off;
  uint32_t* const cnt = (uint32_t*)(wb + w.o_cnt);
  HIP_CHECK(hipMemcpyAsync(wb, blk.data(), m * sizeof(E8Block), hipMemcpyHostToDevice, e.stream));
  hipError_t rc = launch_une8_mark(ob, (const E8Block*)wb, (uint32_t)m, (uint32_t)ntiles, cnt, (uint32_t*)(wb + w.o_st), wb + w.o_tmp, w.tmp_bytes, e.stream);
  if (launch_failed(rc, "device E8E9 filter failed: ", note)) return false;
  uint32_t nseeds = 0, nlist = 0;
  HIP_CHECK(hipMemcpyAsync(&nseeds, cnt + ntiles, 4, hipMemcpyDeviceToHost, e.stream));
  HIP_CHECK(hipMemcpyAsync(&nlist, cnt + 2 * ntiles, 4, hipMemcpyDeviceToHost, e.stream));
  HIP_CHECK(hipStreamSynchronize(e.stream));
  if (nseeds) {
    if (held + 4ull * nlist + (1u << 20) > e.budget) { note = "the filter's list exceeds the device budget"; return false; }
    e.io_in.ensure(4ull * nlist + 64);
    rc = launch_une8_walk(ob, (const E8Block*)wb, (uint32_t)m, (uint32_t)ntiles, cnt, (uint32_t*)e.io_in.p, nseeds, kE8MaxSteps, (uint32_t*)(wb + w.o_st), e.stream);
    if (launch_failed(rc, "device E8E9 filter failed: ", note)) return false;
  }
  HIP_CHECK(hipMemcpyAsync(status.data(), wb + w.o_st, 4 * m, hipMemcpyDeviceToHost, e.stream));
  HIP_CHECK(hipStreamSynchronize(e.stream));
  return true;
}

// The decoded blocks of a batch as the filter takes them: add() those that are live in the order they lie in io_out (i: the
// caller's index of the block), then run() over them.  tiles and ws_bytes(): what the list as it stands asks of the budget.
struct E8List {
  std::vector<E8Block> blk;
  std::vector<size_t> who;
  uint64_t tiles = 0;
  void add(size_t i, uint64_t off, uint32_t n) {
    blk.push_back(E8Block{off, n, (uint32_t)tiles});
    who.push_back(i);
    tiles += e8_tiles(n);
  }
  uint64_t ws_bytes() const { return une8_ws(blk.size(), tiles).bytes; }
  // une8_run over the list; lost[i] = 1 (of `count` caller's blocks): a lane gave block i up.  false + note: as une8_run
  bool run(Engine& e, uint64_t ws_off, uint64_t held, size_t count, std::vector<char>& lost, std::string& note) const {
    std::vector<uint32_t> st;
    lost.assign(count, 0);
    if (!une8_run(e, ws_off, blk, tiles, held, st, note)) return false;
    for (size_t k = 0; k < blk.size(); ++k) if (st[k] != 0) lost[who[k]] = 1;
    return true;
  }
};

// device/lz77_decode_kernel.h for a batch of host streams: one upload, the parse, 12 bytes per stream back, the outputs placed
// back to back (sizes first, then emission: no bound is guessed), the copy, the outputs down.  e8: the method's program filters
// M before it writes it out -- the outputs are placed for device/e8e9_kernel.h, which runs over them before they go down.
static int lz77_decode_batch(U32 level, U32 rb, U32 min_match, U32 mbits, std::vector<StreamJob>& jobs, std::string& note, bool e8) {
  const size_t n = jobs.size();
  if (!n) return 1;
  for (StreamJob& j : jobs) { j.status = 1; j.out_len = 0; }
  if (n > 65535 || (level != 1 && level != 2) || rb > 7 || min_match > 255 || mbits > 32) { note = "batch outside the device decoder's range"; return -1; }
  std::vector<UnlzStream> st(n);
  uint64_t in_bytes = 0, ntok = 0;
  for (size_t i = 0; i < n; ++i) {
    UnlzStream& S = st[i];
    memset(&S, 0, sizeof(S));
    S.in_off = in_bytes;
    S.tok_off = ntok;
    S.in_len = jobs[i].in_len;
    S.tok_cap = jobs[i].in_len;                      // a code has at least 8 bits: at most one token per stream byte
    S.level = level;
    S.rb = rb;
    S.min_match = min_match;
    S.mbits = mbits;
    in_bytes += align_up(jobs[i].in_len, 4);
    ntok += jobs[i].in_len;
  }
  EngineCall call;
  Engine& e = call.e;
  // the arena buffer (idle between batches): tokens, the stream table, the results, where the outputs start
  Carve cv;
  cv.take(16 * ntok);
  const uint64_t o_st = cv.take(n * sizeof(UnlzStream));
  const uint64_t o_res = cv.take(n * sizeof(UnlzResult));
  const uint64_t o_off = cv.take(8 * n);
  const uint64_t ws = cv.at + 256;
  if (ws + in_bytes + (1u << 20) > e.budget) { note = "decoder workspace exceeds the device budget"; return -1; }
  e.io_in.ensure(in_bytes + 64);
  e.arena.ensure(ws);
  uint8_t* const ab = (uint8_t*)e.arena.p;
  std::vector<HostItem> items(n);
  for (size_t i = 0; i < n; ++i) items[i] = HostItem{jobs[i].in, jobs[i].in_len, st[i].in_off};
  const auto staged = upload_staged(e, e.io_in.p, items, in_bytes, 4, false);
  HIP_CHECK(hipMemcpyAsync(ab + o_st, st.data(), n * sizeof(UnlzStream), hipMemcpyHostToDevice, e.stream));
  hipError_t rc = launch_unlz_parse((const uint8_t*)e.io_in.p, (const UnlzStream*)(ab + o_st), (uint32_t)n, ab, (UnlzResult*)(ab + o_res), e.stream);
  if (launch_failed(rc, "device LZ77 decoder failed: ", note)) return -1;
  std::vector<UnlzResult> res(n);
  HIP_CHECK(hipMemcpyAsync(res.data(), ab + o_res, n * sizeof(UnlzResult), hipMemcpyDeviceToHost, e.stream));
  HIP_CHECK(hipStreamSynchronize(e.stream));
  std::vector<uint64_t> off(n);
  uint64_t room = 0;
  bool fits = true, any = false;
  E8List fl;                                        // e8: the decoded blocks as the filter sees them
  for (size_t i = 0; i < n; ++i) {
    off[i] = room;
    if (res[i].status != kUnlzOk) continue;
    jobs[i].out_len = res[i].out_len;
    if (e8) fl.add(i, room, res[i].out_len);
    room += e8 ? e8_room(res[i].out_len) : res[i].out_len;
    any = true;
    if (!jobs[i].vec && res[i].out_len > jobs[i].cap) fits = false;
  }
  if (room > (1ull << 31)) { note = "more than 2 GiB of output in one batch"; return declined(jobs); }
  const uint64_t f_off = e8 ? align_up(room, 256) : room, f_ws = e8 ? fl.ws_bytes() : 0;
  if (ws + in_bytes + f_off + f_ws + (1u << 20) > e.budget) { note = "the decoded blocks exceed the device budget"; return declined(jobs); }
  if (!fits) return 0;
  if (any) {
    e.io_out.ensure(f_off + f_ws + 64);
    HIP_CHECK(hipMemcpyAsync(ab + o_off, off.data(), 8 * n, hipMemcpyHostToDevice, e.stream));
    rc = launch_unlz_copy((const uint8_t*)e.io_in.p, (const UnlzStream*)(ab + o_st), (uint32_t)n, ab, (const UnlzResult*)(ab + o_res),
                          (const uint64_t*)(ab + o_off), (uint8_t*)e.io_out.p, e.stream);
    if (launch_failed(rc, "device LZ77 decoder failed: ", note)) return declined(jobs);
    if (e8) {
      std::vector<char> lost;
      if (!fl.run(e, f_off, ws + f_off + f_ws, n, lost, note)) return declined(jobs);
      for (size_t i = 0; i < n; ++i) if (lost[i]) { res[i].status = kUnlzLong; jobs[i].out_len = 0; }
    }
    for (size_t i = 0; i < n; ++i) {
      if (res[i].status != kUnlzOk) continue;
      deliver(e, jobs[i], off[i], res[i].out_len);
    }
    HIP_CHECK(hipStreamSynchronize(e.stream));
  }
  for (size_t i = 0; i < n; ++i) if (res[i].status == kUnlzOk) jobs[i].status = 0;
  return 1;
}
int engine_lz77_decode(U32 level, U32 rb, U32 min_match, U32 mbits, std::vector<StreamJob>& jobs, std::string& note) {
  return lz77_decode_batch(level, rb, min_match, mbits, jobs, note, false);
}

// device/lz77_decode_wide_kernel.h for a batch of host streams.  Streams who[0 .. m) of `jobs` as one batch on the
// device: the upload, the pieces' parses, the stitch and the final lists; 40 bytes per stream back, the counts among them; the outputs
// placed back to back (sizes first, then emission: no bound is guessed); a word per output byte linked, jumped until a round
// changes nothing, emitted; the outputs down.  kUnlzwRan: status and out_len of its jobs are final.  kUnlzwShort: some decoded
// block does not fit its job's buffer -- every out_len is reported, nothing was written.  Otherwise nothing was delivered either
// and `note` says why -- kUnlzwOver: the batch does not fit the budget or 2 GiB of output; kUnlzwBroken: a launch failed.
// P.e8: the method's program filters M before it writes it out (x.,5 / x.,6).  Link and jump run over the packed outputs as ever;
// the bytes are emitted into rooms placed for device/e8e9_kernel.h (io_out: the rooms, each on a multiple of kE8Lane and rounded up
// to one; then w; then the filter's workspace), which runs over them before anything goes down.  An empty output is delivered as
// empty and never enters the filter's list; a block a lane of the walk gave up is declined (status 1, out_len 0).
namespace {
enum { kUnlzwBroken = -1, kUnlzwOver = 0, kUnlzwRan = 1, kUnlzwShort = 2 };
struct UnlzWideParams { U32 level, rb, min_match, mbits, piece; bool e8; };
std::atomic<U32> g_last_unlz_wide_pieces[4], g_last_unlz_wide_rounds{0};

// what a stream holds on the device before its size is known: the slots of three arrays and the stream
uint64_t unlz_wide_slots(U32 in_len, U32 piece) { return ((uint64_t)in_len + piece - 1) / piece * piece; }
// (e8: the room's padding, the block's entry and status, the counts of its first tile -- the rest of the filter's workspace, 8 bytes per
// 4 KiB of output, is known only with the sizes)
uint64_t unlz_wide_e8_need() { return kE8Lane + sizeof(E8Block) + 4 + 8; }
uint64_t unlz_wide_need(U32 in_len, U32 piece, bool e8) {
  return 36 * unlz_wide_slots(in_len, piece) + align_up(in_len, 4) + 256 + (e8 ? unlz_wide_e8_need() : 0);
}

int unlz_wide_run(Engine& e, const UnlzWideParams& P, std::vector<StreamJob>& jobs, const size_t* who, size_t m, U32 counts[4], U32& rounds, std::string& note) {
  std::vector<UnlzWideStream> st(m);
  std::vector<UnlzWideRef> refs;
  uint64_t in_bytes = 0, slots = 0;
  for (size_t k = 0; k < m; ++k) {
    UnlzWideStream& S = st[k];
    memset(&S, 0, sizeof(S));
    S.in_off = in_bytes;
    S.tok_off = slots;
    S.in_len = jobs[who[k]].in_len;
    S.piece0 = (uint32_t)refs.size();
    S.npieces = (uint32_t)(unlz_wide_slots(S.in_len, P.piece) / P.piece);
    S.level = P.level;
    S.rb = P.rb;
    S.min_match = P.min_match;
    S.mbits = P.mbits;
    for (uint32_t i = 0; i < S.npieces; ++i) refs.push_back(UnlzWideRef{(uint32_t)k, i});
    in_bytes += align_up(S.in_len, 4);
    slots += (uint64_t)S.npieces * P.piece;
  }
  const size_t np = refs.size();
  // the arena buffer (idle between batches): the pieces' tokens, the final lists, the start states, the tables
  Carve cv;
  cv.take(16 * slots);
  const uint64_t o_fin = cv.take(16 * slots);
  const uint64_t o_states = cv.take(4 * slots);
  const uint64_t o_pieces = cv.take(np * sizeof(UnlzWidePieceOut));
  const uint64_t o_adopt = cv.take(np * sizeof(UnlzWideAdopt));
  const uint64_t o_refs = cv.take(np * sizeof(UnlzWideRef));
  const uint64_t o_st = cv.take(m * sizeof(UnlzWideStream));
  const uint64_t o_outs = cv.take(m * sizeof(UnlzWideOut));
  const uint64_t o_place = cv.take(m * sizeof(UnlzWidePlace));
  const uint64_t o_dst = P.e8 ? cv.take(8 * m) : 0;
  const uint64_t o_flags = cv.take(4 * kUnlzWideRounds);
  const uint64_t ws = cv.at + 256;
  const uint64_t f_least = P.e8 ? kE8Lane * (uint64_t)m + une8_ws(m, m).bytes : 0;      // were every output one tile
  if (ws + in_bytes + f_least + (1u << 20) > e.budget) { note = "decoder workspace exceeds the device budget"; return kUnlzwOver; }
  e.io_in.ensure(in_bytes + 64);
  e.arena.ensure(ws);
  uint8_t* const ab = (uint8_t*)e.arena.p;
  std::vector<HostItem> items(m);
  for (size_t k = 0; k < m; ++k) items[k] = HostItem{jobs[who[k]].in, jobs[who[k]].in_len, st[k].in_off};
  const auto staged = upload_staged(e, e.io_in.p, items, in_bytes, 4, false);
  HIP_CHECK(hipMemcpyAsync(ab + o_st, st.data(), m * sizeof(UnlzWideStream), hipMemcpyHostToDevice, e.stream));
  if (np) HIP_CHECK(hipMemcpyAsync(ab + o_refs, refs.data(), np * sizeof(UnlzWideRef), hipMemcpyHostToDevice, e.stream));
  const uint8_t* const in_all = (const uint8_t*)e.io_in.p;
  const UnlzWideStream* const d_st = (const UnlzWideStream*)(ab + o_st);
  hipError_t rc = launch_unlz_wide_parse(P.level, in_all, d_st, (uint32_t)m, (const UnlzWideRef*)(ab + o_refs), (uint32_t)np, P.piece, ab, (uint32_t*)(ab + o_states),
                                         (UnlzWidePieceOut*)(ab + o_pieces), ab + o_fin, (UnlzWideAdopt*)(ab + o_adopt), (UnlzWideOut*)(ab + o_outs),
                                         e.stream);
  if (launch_failed(rc, "device LZ77 decoder failed: ", note)) return kUnlzwBroken;
  std::vector<UnlzWideOut> outs(m);
  HIP_CHECK(hipMemcpyAsync(outs.data(), ab + o_outs, m * sizeof(UnlzWideOut), hipMemcpyDeviceToHost, e.stream));
  HIP_CHECK(hipStreamSynchronize(e.stream));
  std::vector<UnlzResult> res(m);
  std::vector<UnlzWidePlace> place;
  std::vector<uint64_t> off(m), dst;
  uint64_t room = 0, placed = 0;                    // the outputs packed (w's index space); in their rooms (e8: aligned, else the same)
  bool fits = true;
  E8List fl;                                        // e8: the decoded, non-empty blocks as the filter sees them
  for (size_t k = 0; k < m; ++k) {
    StreamJob& j = jobs[who[k]];
    const UnlzWideStats& c = outs[k].stats;
    res[k] = outs[k].r;
    if (outs[k].err != ~0ull) res[k].status = (uint32_t)(outs[k].err & 7u);        // the first token that failed a position check
    counts[0] += c.pieces; counts[1] += c.entered; counts[2] += c.met; counts[3] += c.walked;
    off[k] = placed;
    if (res[k].status != kUnlzOk) continue;
    j.out_len = res[k].out_len;
    if (res[k].out_len) {
      place.push_back(UnlzWidePlace{room, res[k].out_len, res[k].ntok, (uint32_t)k, 0u});
      if (P.e8) { dst.push_back(placed); fl.add(k, placed, res[k].out_len); }
    }
    room += res[k].out_len;
    placed += P.e8 ? e8_room(res[k].out_len) : res[k].out_len;
    if (!j.vec && res[k].out_len > j.cap) fits = false;
  }
  if (placed > (1ull << 31)) { note = "more than 2 GiB of output in one batch"; return kUnlzwOver; }
  const uint64_t w_off = align_up(placed, 256);
  const uint64_t f_off = P.e8 ? align_up(w_off + 4 * room, 256) : w_off + 4 * room, f_ws = P.e8 ? fl.ws_bytes() : 0;
  if (ws + in_bytes + f_off + f_ws + (1u << 20) > e.budget) { note = "the decoded blocks exceed the device budget"; return kUnlzwOver; }
  if (!fits) return kUnlzwShort;
  if (room) {
    e.io_out.ensure(f_off + f_ws + 64);
    uint32_t* const w = (uint32_t*)((uint8_t*)e.io_out.p + w_off);
    uint32_t* const d_flags = (uint32_t*)(ab + o_flags);
    HIP_CHECK(hipMemcpyAsync(ab + o_place, place.data(), place.size() * sizeof(UnlzWidePlace), hipMemcpyHostToDevice, e.stream));
    HIP_CHECK(hipMemsetAsync(d_flags, 0, 4 * kUnlzWideRounds, e.stream));
    rc = launch_unlz_wide_link(in_all, d_st, (const UnlzWidePlace*)(ab + o_place), (uint32_t)place.size(), (uint32_t)room, ab + o_fin, w, e.stream);
    if (launch_failed(rc, "device LZ77 decoder failed: ", note)) return kUnlzwBroken;
    for (uint32_t r = 0;; ++r) {
      if (r == kUnlzWideRounds) { note = "the copy did not settle within the bound of jump rounds"; return kUnlzwOver; }
      rc = launch_unlz_wide_jump(w, (uint32_t)room, d_flags + r, e.stream);
      if (launch_failed(rc, "device LZ77 decoder failed: ", note)) return kUnlzwBroken;
      uint32_t more = 0;
      HIP_CHECK(hipMemcpyAsync(&more, d_flags + r, 4, hipMemcpyDeviceToHost, e.stream));
      HIP_CHECK(hipStreamSynchronize(e.stream));
      if (r + 1 > rounds) rounds = r + 1;
      if (!more) break;
    }
    if (P.e8) {
      HIP_CHECK(hipMemcpyAsync(ab + o_dst, dst.data(), 8 * dst.size(), hipMemcpyHostToDevice, e.stream));
      rc = launch_unlz_wide_emit_placed(w, (const UnlzWidePlace*)(ab + o_place), (const uint64_t*)(ab + o_dst), (uint32_t)place.size(), (uint32_t)room,
                                        (uint8_t*)e.io_out.p, e.stream);
    } else rc = launch_unlz_wide_emit(w, (uint32_t)room, (uint8_t*)e.io_out.p, e.stream);
    if (launch_failed(rc, "device LZ77 decoder failed: ", note)) return kUnlzwBroken;
    if (P.e8) {                                     // (the streams in io_in are dead from here on: the filter's list goes there)
      std::vector<char> lost;
      // (a list beyond the budget is this batch's size, no failure of the device)
      if (!fl.run(e, f_off, ws + f_off + f_ws, m, lost, note)) return note.find("budget") == std::string::npos ? kUnlzwBroken : kUnlzwOver;
      for (size_t k = 0; k < m; ++k) if (lost[k]) { res[k].status = kUnlzLong; jobs[who[k]].out_len = 0; }
    }
  }
  for (size_t k = 0; k < m; ++k) if (res[k].status == kUnlzOk) deliver(e, jobs[who[k]], off[k], res[k].out_len);
  HIP_CHECK(hipStreamSynchronize(e.stream));
  for (size_t k = 0; k < m; ++k) if (res[k].status == kUnlzOk) jobs[who[k]].status = 0;
  return kUnlzwRan;
}
}  // namespace

void engine_last_unlz_wide_pieces(U32 out[4]) { for (int k = 0; k < 4; ++k) out[k] = g_last_unlz_wide_pieces[k].load(std::memory_order_relaxed); }
U32 engine_last_unlz_wide_rounds() { return g_last_unlz_wide_rounds.load(std::memory_order_relaxed); }

// The batch as one when it fits.  Jobs that all deliver into vectors (an archive's segments) may be cut: consecutive sub-batches
// by what they hold before their sizes are known, and a sub-batch whose decoded blocks then exceed the budget or 2 GiB runs again
// stream by stream; only a stream that does not fit alone is declined (status 1; -1 + note when nothing else was decoded).  Jobs
// with buffers of their own run as one batch or not at all: nothing may be written before every size is known.  After a failed
// launch nothing more is started.
static int lz77_decode_wide_batch(U32 level, U32 rb, U32 min_match, U32 mbits, std::vector<StreamJob>& jobs, std::string& note, bool e8) {
  const size_t n = jobs.size();
  for (int k = 0; k < 4; ++k) g_last_unlz_wide_pieces[k].store(0, std::memory_order_relaxed);
  g_last_unlz_wide_rounds.store(0, std::memory_order_relaxed);
  if (!n) return 1;
  bool all_vec = true;
  for (StreamJob& j : jobs) { j.status = 1; j.out_len = 0; all_vec = all_vec && j.vec; }
  if (n > 65535 || (level != 1 && level != 2) || rb > 7 || min_match > 255 || mbits > 32) { note = "batch outside the device decoder's range"; return -1; }
  U64 piece = kUnlzWidePiece;
  if (const char* v = getenv("ZPAQ_AMD_UNLZ_WIDE_PIECE")) { const long long x = atoll(v); if (x > 0) piece = (U64)x; }
  const UnlzWideParams P{level, rb, min_match, mbits, unlz_wide_piece_clamped(piece), e8};
  std::vector<size_t> who(n);
  for (size_t i = 0; i < n; ++i) who[i] = i;
  U32 counts[4] = {0, 0, 0, 0}, rounds = 0;
  bool some = false, left = false, broken = false;
  EngineCall call;
  Engine& e = call.e;
  auto drop = [&](size_t from, size_t end) { left = true; for (size_t i = from; i < end; ++i) { jobs[i].out_len = 0; jobs[i].status = 1; } };
  for (size_t from = 0; from < n && !broken;) {
    size_t end = n;
    if (all_vec) {
      uint64_t need = 0;
      for (end = from; end < n; ++end) {
        need += unlz_wide_need(jobs[end].in_len, P.piece, e8);
        if (end > from && need > e.budget / 2) break;
      }
    }
    int ran = unlz_wide_run(e, P, jobs, who.data() + from, end - from, counts, rounds, note);
    if (ran == kUnlzwShort) return 0;                       // (one batch: nothing was written)
    if (ran == kUnlzwOver && all_vec && end - from > 1) {
      for (size_t i = from; i < end && !broken; ++i) {
        ran = unlz_wide_run(e, P, jobs, who.data() + i, 1, counts, rounds, note);
        if (ran == kUnlzwRan) some = true; else drop(i, i + 1);
        if (ran == kUnlzwBroken) { broken = true; drop(i + 1, n); }
      }
    } else if (ran == kUnlzwRan) some = true;
    else {
      drop(from, end);
      if (ran == kUnlzwBroken) { broken = true; drop(end, n); }
    }
    from = end;
  }
  for (int k = 0; k < 4; ++k) g_last_unlz_wide_pieces[k].store(counts[k], std::memory_order_relaxed);
  g_last_unlz_wide_rounds.store(rounds, std::memory_order_relaxed);
  if (left && !some) return declined(jobs);
  return 1;
}
int engine_lz77_decode_wide(U32 level, U32 rb, U32 min_match, U32 mbits, std::vector<StreamJob>& jobs, std::string& note) {
  return lz77_decode_wide_batch(level, rb, min_match, mbits, jobs, note, false);
}
int engine_e8e9_decode_wide(int kind, U32 rb, U32 min_match, U32 mbits, std::vector<StreamJob>& jobs, std::string& note) {
  if (kind != 5 && kind != 6) {
    for (StreamJob& j : jobs) { j.status = 1; j.out_len = 0; }
    note = "batch outside the device decoder's range";
    return -1;
  }
  return lz77_decode_wide_batch((U32)(kind - 4), rb, min_match, mbits, jobs, note, true);
}

// The BWT decoders, device/bwt_decode_kernel.h (4-byte nodes, blocks below 16 MiB) and device/bwt_decode_wide_kernel.h (8-byte
// nodes, the program at args[0] 5 .. 11), for a batch of host streams.  The host admits the streams (the rule, the range), so
// every size is known and the room is checked before anything runs; then one upload, the kernels, a word per stream back, and the
// outputs of the streams whose path was whole down.  e8: as for lz77_decode_batch.

// The host's step: admitted stream k is jobs[who[k]], n[k] bytes (reported in out_len) with the marker at idx[k]; empty[i]: job i
// is the empty block's stream; fits: every admitted stream has room in its job's buffer
struct BwtAdmitted {
  std::vector<size_t> who;
  std::vector<uint32_t> n, idx;
  std::vector<char> empty;
  bool fits = true;
};
static BwtAdmitted bwt_admit(bool wide, U32 mbits, std::vector<StreamJob>& jobs) {
  BwtAdmitted a;
  a.empty.assign(jobs.size(), 0);
  for (size_t i = 0; i < jobs.size(); ++i) {
    StreamJob& j = jobs[i];
    if (bwt_stream_empty(j.in, j.in_len)) { a.empty[i] = 1; continue; }
    uint32_t sn = 0, sidx = 0;
    if (!(wide ? bwt_wide_stream_admitted(j.in, j.in_len, mbits, sn, sidx) : bwt_stream_admitted(j.in, j.in_len, mbits, sn, sidx))) continue;
    j.out_len = sn;
    if (!j.vec && sn > j.cap) a.fits = false;
    a.who.push_back(i);
    a.n.push_back(sn);
    a.idx.push_back(sidx);
  }
  return a;
}
// the call's end when the device did its part: the empty blocks' streams are decoded too
static int bwt_done(std::vector<StreamJob>& jobs, const BwtAdmitted& a) {
  for (size_t i = 0; i < jobs.size(); ++i) if (a.empty[i]) { if (jobs[i].vec) jobs[i].vec->clear(); jobs[i].status = 0; }
  return 1;
}

// Admitted streams from .. end as one batch on the device (layout.h BwtNeed): st[k] and s2[k] are stream from + k's
struct BwtPlaced {
  BwtNeed w;
  std::vector<BwtStream> st;
  std::vector<uint32_t> s2;                         // where the streams' second-level tables start (the wide form's)
};
static BwtPlaced bwt_place(const BwtAdmitted& a, size_t from, size_t end, bool e8) {
  BwtPlaced p;
  p.st.resize(end - from);
  p.s2.resize(end - from);
  for (size_t k = 0; k < end - from; ++k) p.st[k] = p.w.place(a.n[from + k], a.idx[from + k], e8, &p.s2[k]);
  return p;
}

// One placed batch of either width, stream k of which is jobs[who[k]]: carve the arena, check the budget, stage, launch, read
// the statuses, filter, deliver.  kBwtRan: status and out_len of its jobs are final.  Otherwise nothing of it was delivered and
// `note` says why -- kBwtOver: it does not fit the budget; kBwtBroken: a launch or the runtime failed.
enum { kBwtBroken = -1, kBwtOver = 0, kBwtRan = 1 };
static int bwt_run(Engine& e, bool wide, bool e8, std::vector<StreamJob>& jobs, const size_t* who, const BwtPlaced& p, std::string& note) {
  const size_t m = p.st.size();
  const BwtNeed& w = p.w;
  // the arena buffer (idle between batches): the list, the tile histograms, the splitter tables, the stream tables, the statuses
  Carve cv;
  cv.take((wide ? 8 : 4) * w.nodes);
  const uint64_t o_hist = cv.take(1024 * w.tiles);
  const uint64_t o_sp = cv.take(16 * w.splits);
  const uint64_t o_sp2 = wide ? cv.take(16 * w.splits2) : 0;
  const uint64_t o_st = cv.take(m * sizeof(BwtStream));
  const uint64_t o_s2 = wide ? cv.take(4 * m) : 0;
  const uint64_t o_res = cv.take(4 * m);
  const uint64_t ws = cv.at + 256;
  uint64_t f_tiles = 0;                             // e8: the filter's tiles, were every stream decoded
  for (size_t k = 0; k < m && e8; ++k) f_tiles += e8_tiles(p.st[k].n);
  const uint64_t f_off = e8 ? align_up(w.room, 256) : w.room, f_ws = e8 ? une8_ws(m, f_tiles).bytes : 0;
  if (ws + w.in_bytes + f_off + f_ws + (1u << 20) > e.budget) { note = "decoder workspace exceeds the device budget"; return kBwtOver; }
  e.io_in.ensure(w.in_bytes + 64);
  e.io_out.ensure(f_off + f_ws + 64);
  e.arena.ensure(ws);
  uint8_t* const ab = (uint8_t*)e.arena.p;
  std::vector<HostItem> items(m);
  for (size_t k = 0; k < m; ++k) items[k] = HostItem{jobs[who[k]].in, jobs[who[k]].in_len, p.st[k].in_off};
  const auto staged = upload_staged(e, e.io_in.p, items, w.in_bytes, 4, false);
  HIP_CHECK(hipMemcpyAsync(ab + o_st, p.st.data(), m * sizeof(BwtStream), hipMemcpyHostToDevice, e.stream));
  if (wide) HIP_CHECK(hipMemcpyAsync(ab + o_s2, p.s2.data(), 4 * m, hipMemcpyHostToDevice, e.stream));
  const uint8_t* const in_all = (const uint8_t*)e.io_in.p;
  const BwtStream* const d_st = (const BwtStream*)(ab + o_st);
  uint32_t* const d_hist = (uint32_t*)(ab + o_hist);
  uint32_t* const d_res = (uint32_t*)(ab + o_res);
  const hipError_t rc =
      wide ? launch_bwt_decode_wide(in_all, d_st, (const uint32_t*)(ab + o_s2), (uint32_t)m, (uint32_t)w.tiles, (uint32_t)w.splits, (uint32_t)w.splits2,
                                    d_hist, (uint64_t*)ab, ab + o_sp, ab + o_sp2, d_res, (uint8_t*)e.io_out.p, e.stream)
           : launch_bwt_decode(in_all, d_st, (uint32_t)m, (uint32_t)w.tiles, (uint32_t)w.splits, d_hist, (uint32_t*)ab, ab + o_sp, d_res,
                               (uint8_t*)e.io_out.p, e.stream);
  if (launch_failed(rc, "device BWT decoder failed: ", note)) return kBwtBroken;
  std::vector<uint32_t> res(m);
  HIP_CHECK(hipMemcpyAsync(res.data(), ab + o_res, 4 * m, hipMemcpyDeviceToHost, e.stream));
  HIP_CHECK(hipStreamSynchronize(e.stream));
  if (e8) {
    E8List fl;
    std::vector<char> lost;
    for (size_t k = 0; k < m; ++k) if (res[k] == 0) fl.add(k, p.st[k].out_off, p.st[k].n);
    // (a list beyond the budget is this batch's size, no failure of the device)
    if (!fl.run(e, f_off, ws + f_off + f_ws, m, lost, note)) return note.find("budget") == std::string::npos ? kBwtBroken : kBwtOver;
    for (size_t k = 0; k < m; ++k) if (lost[k]) res[k] = 1u;
  }
  for (size_t k = 0; k < m; ++k) {
    StreamJob& j = jobs[who[k]];
    if (res[k] != 0) { j.out_len = 0; continue; }
    deliver(e, j, p.st[k].out_off, p.st[k].n);
  }
  HIP_CHECK(hipStreamSynchronize(e.stream));
  for (size_t k = 0; k < m; ++k) if (res[k] == 0) jobs[who[k]].status = 0;
  return kBwtRan;
}

// The small form: the batch as a whole or not at all -- whatever keeps it from running declines it (-1 + note).
static int bwt_decode_batch(U32 mbits, std::vector<StreamJob>& jobs, std::string& note, bool e8) {
  const size_t n = jobs.size();
  if (!n) return 1;
  for (StreamJob& j : jobs) { j.status = 1; j.out_len = 0; }
  if (n > 65535 || mbits > 32) { note = "batch outside the device decoder's range"; return -1; }
  const BwtAdmitted a = bwt_admit(false, mbits, jobs);
  const BwtPlaced p = bwt_place(a, 0, a.who.size(), e8);
  if (p.w.room > (1ull << 31)) { note = "more than 2 GiB of output in one batch"; return declined(jobs); }
  if (!a.fits) return 0;
  if (!a.who.empty()) {
    EngineCall call;
    if (bwt_run(call.e, false, e8, jobs, a.who.data(), p, note) != kBwtRan) return declined(jobs);
  }
  return bwt_done(jobs, a);
}
int engine_bwt_decode(U32 mbits, std::vector<StreamJob>& jobs, std::string& note) { return bwt_decode_batch(mbits, jobs, note, false); }

// The wide form (mbits 25 .. 31).  These blocks are large: a batch whose outputs exceed 2 GiB or whose workspace exceeds the budget
// is cut into consecutive sub-batches that each fit (layout.h bwt_wide_cut), which run one after the other through the same
// buffers.  Only a stream that does not fit alone is declined (status 1 + note; -1 when nothing else was decoded either).  After a
// failed launch nothing more is started: that sub-batch and every stream behind it are declined.
static int bwt_decode_wide_batch(U32 mbits, std::vector<StreamJob>& jobs, std::string& note, bool e8) {
  const size_t n = jobs.size();
  if (!n) return 1;
  for (StreamJob& j : jobs) { j.status = 1; j.out_len = 0; }
  if (mbits < 25 || mbits > 31) { note = "batch outside the device decoder's range"; return -1; }
  const BwtAdmitted a = bwt_admit(true, mbits, jobs);
  if (!a.fits) return 0;
  const size_t m = a.who.size();
  bool some = false, left = false;
  if (m) {
    EngineCall call;
    Engine& e = call.e;
    // (the filter's own tables are about 8 bytes per 4 KiB tile: the cut leaves them 1/256 of the budget)
    const uint64_t spare = (1u << 20) + (e8 ? e.budget / 256 : 0), held_limit = e.budget > spare ? e.budget - spare : 0;
    for (size_t from = 0; from < m;) {
      size_t end = bwt_wide_cut(a.n.data(), m, from, 1ull << 31, held_limit, e8);
      int ran = kBwtOver;
      if (end == from) { note = "decoder workspace exceeds the device budget"; end = from + 1; }
      else ran = bwt_run(e, true, e8, jobs, a.who.data() + from, bwt_place(a, from, end, e8), note);
      if (ran == kBwtRan) some = true;
      else { left = true; for (size_t k = from; k < end; ++k) jobs[a.who[k]].out_len = 0; }
      from = end;
      if (ran == kBwtBroken) {                          // only a sub-batch beyond the budget lets the next one run
        for (size_t k = from; k < m; ++k) jobs[a.who[k]].out_len = 0;
        break;
      }
    }
  }
  if (left && !some) return declined(jobs);
  return bwt_done(jobs, a);
}
int engine_bwt_decode_wide(U32 mbits, bool e8, std::vector<StreamJob>& jobs, std::string& note) { return bwt_decode_wide_batch(mbits, jobs, note, e8); }

// Streams of the E8E9 methods back into their blocks: the stage in front with the method's own parameters (kind 5 / 6: the LZ77
// decoder, kind 7: the BWT decoder, kind 4: none -- the stream is the filtered block), then device/e8e9_kernel.h over its output
// while that is still on the device.
int engine_e8e9_decode(int kind, U32 rb, U32 min_match, U32 mbits, std::vector<StreamJob>& jobs, std::string& note) {
  if (kind == 5 || kind == 6) return lz77_decode_batch((U32)(kind - 4), rb, min_match, mbits, jobs, note, true);
  if (kind == 7) return bwt_decode_batch(mbits, jobs, note, true);
  const size_t n = jobs.size();
  if (!n) return 1;
  for (StreamJob& j : jobs) { j.status = 1; j.out_len = 0; }
  if (n > 65535 || kind != 4) { note = "batch outside the device filter's range"; return -1; }
  E8List fl;                                        // every stream is a block: fl.blk[i] is jobs[i]
  uint64_t room = 0;
  bool fits = true;
  for (size_t i = 0; i < n; ++i) {
    fl.add(i, room, jobs[i].in_len);
    room += e8_room(jobs[i].in_len);
    jobs[i].out_len = jobs[i].in_len;
    if (!jobs[i].vec && jobs[i].in_len > jobs[i].cap) fits = false;
  }
  if (room > (1ull << 31)) { note = "more than 2 GiB of output in one batch"; return declined(jobs); }
  if (!fits) return 0;
  EngineCall call;
  Engine& e = call.e;
  const uint64_t f_off = align_up(room, 256), f_ws = fl.ws_bytes();
  if (f_off + f_ws + (1u << 20) > e.budget) { note = "the blocks exceed the device budget"; return declined(jobs); }
  e.io_out.ensure(f_off + f_ws + 64);
  std::vector<HostItem> items(n);
  for (size_t i = 0; i < n; ++i) items[i] = HostItem{jobs[i].in, jobs[i].in_len, fl.blk[i].off};
  const auto staged = upload_staged(e, e.io_out.p, items, room, kE8Lane, false);      // (the rooms: e8_room rounds up to a lane's bytes)
  std::vector<char> lost;
  if (!fl.run(e, f_off, f_off + f_ws, n, lost, note)) return declined(jobs);
  for (size_t i = 0; i < n; ++i) {
    StreamJob& j = jobs[i];
    if (lost[i]) { j.out_len = 0; continue; }
    deliver(e, j, fl.blk[i].off, j.in_len);
  }
  HIP_CHECK(hipStreamSynchronize(e.stream));
  for (size_t i = 0; i < n; ++i) if (!lost[i]) jobs[i].status = 0;
  return 1;
}

}  // namespace zpq
