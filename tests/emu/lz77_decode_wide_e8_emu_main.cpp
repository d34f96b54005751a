// TEST INFRASTRUCTURE -- streams of the E8E9 forms of the LZ77 methods back into their blocks: the decoder that parses a stream in
// pieces (zpaq_amd/csrc/device/lz77_decode_wide_kernel.h) and the inverse filter behind it (zpaq_amd/csrc/device/e8e9_kernel.h) on
// the host-side wavefront emulator (wave_emu.h), doing what the engine does: the piece parse, the stitch, the finalize step; the
// host's placement -- the outputs packed for link and jump, and in rooms on multiples of 16 bytes for the filter --; link, the
// jump rounds, unlzw_emit_placed_body into the rooms; then mark, the scan over the tiles' counts as a host loop, scatter and walk.
// Every array has its exact size between inaccessible pages (guard_alloc.h) and starts dirty.  The kernels of a lane per element
// run thread after thread in the order ZPQ_EMU_ORDER says; the others are the emulator's workgroups, which read it themselves.
//
//   lz77_decode_wide_e8_emu <level> <rb> <min_match> <mbits> <piece> <max_steps> <out_prefix> <stream>...
//                                                                          max_steps 0: the engine's cap (kE8MaxSteps)
//
// Prints "stream <k> status <s> out_len <n> ntok <t> listed <0|1>" per stream (listed: the stream's output was in the filter's
// list; a block the walk gave up has status 1 and out_len 0), "pieces <all> <entered> <met> <walked>", "rounds <r>", "launches
// <n>" (the kernels started behind the host's placement: none over an empty total) and "edges ok" (the byte in front of the first
// room is as it was; the last room ends where an inaccessible page starts).  <out_prefix>.<k> = stream k's block, for status 0.
#include "wave_emu.h"

#include <string>
#include <vector>

#include "guard_alloc.h"

// (fibers of one OS thread, switched only at cross-lane operations: a plain read-modify-write is atomic)
static inline unsigned long long atomicMin(unsigned long long* p, unsigned long long v) { const unsigned long long old = *p; if (v < old) *p = v; return old; }

#include "e8e9_kernel.h"
#include "lz77_decode_wide_kernel.h"

namespace {

std::vector<uint8_t> slurp(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}

struct Args {
  const uint8_t* in_all;
  const zpq::UnlzWideStream* streams;
  const zpq::UnlzWideRef* refs;
  uint32_t piece;
  uint4* prov;
  uint32_t* states;
  zpq::UnlzWidePieceOut* pieces;
  uint4* fin;
  zpq::UnlzWideAdopt* adopt;
  zpq::UnlzWideOut* outs;
  // the filter
  uint8_t* buf;
  const zpq::E8Block* blocks;
  uint32_t nblocks, ntiles, nseeds, max_steps;
  uint32_t* cnt;
  uint32_t* list;
  uint32_t* status;
};

template <bool kBits>
void piece_thunk(void* p) { Args* a = (Args*)p; zpq::unlzw_piece_body<kBits>(a->in_all, a->streams, a->refs, a->piece, a->prov, a->states, a->pieces); }
template <bool kBits>
void stitch_thunk(void* p) {
  Args* a = (Args*)p;
  zpq::unlzw_stitch_body<kBits>(a->in_all, a->streams, a->piece, a->prov, a->states, a->pieces, a->fin, a->adopt, a->outs);
}
void mark_thunk(void* p) { Args* a = (Args*)p; zpq::une8_mark_body(a->buf, a->blocks, a->nblocks, a->ntiles, a->cnt, a->status); }
void scatter_thunk(void* p) { Args* a = (Args*)p; zpq::une8_scatter_body(a->buf, a->blocks, a->nblocks, a->ntiles, a->cnt, a->list); }
void walk_thunk(void* p) {
  Args* a = (Args*)p;
  zpq::une8_walk_body(a->buf, a->blocks, a->nblocks, a->ntiles, a->cnt, a->list, a->nseeds, a->max_steps, a->status);
}

// a kernel of independent lanes: body() once per thread of `blocks` workgroups of 256
template <class F>
void each_thread(uint64_t blocks, F body) {
  const char* order = getenv("ZPQ_EMU_ORDER");
  const bool reverse = order && !strncmp(order, "reverse", 7);
  for (uint64_t i = 0; i < blocks * 256; ++i) {
    const uint64_t k = reverse ? blocks * 256 - 1 - i : i;
    emu::g_blockIdx = emu::Dim3{(unsigned)(k / 256), 0, 0};
    emu::g_threadIdx = emu::Dim3{(unsigned)(k % 256), 0, 0};
    body();
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 9) {
    fprintf(stderr, "usage: lz77_decode_wide_e8_emu <level> <rb> <min_match> <mbits> <piece> <max_steps> <out_prefix> <stream>...\n");
    return 2;
  }
  const uint32_t level = (uint32_t)atoi(argv[1]), rb = (uint32_t)atoi(argv[2]), min_match = (uint32_t)atoi(argv[3]), mbits = (uint32_t)atoi(argv[4]);
  const uint32_t piece = zpq::unlz_wide_piece_clamped((uint64_t)atoll(argv[5]));
  const uint32_t max_steps = atoi(argv[6]) > 0 ? (uint32_t)atoi(argv[6]) : zpq::kE8MaxSteps;
  const std::string prefix = argv[7];
  const unsigned nb = (unsigned)(argc - 8);
  std::vector<std::vector<uint8_t>> in(nb);
  std::vector<zpq::UnlzWideStream> st(nb);
  std::vector<zpq::UnlzWideRef> rf;
  uint64_t total_in = 0, slots = 0;
  for (unsigned b = 0; b < nb; ++b) {
    in[b] = slurp(argv[8 + b]);
    zpq::UnlzWideStream& S = st[b];
    memset(&S, 0, sizeof S);
    S.in_off = total_in;
    S.tok_off = slots;
    S.in_len = (uint32_t)in[b].size();
    S.piece0 = (uint32_t)rf.size();
    S.npieces = (uint32_t)(((uint64_t)S.in_len + piece - 1) / piece);
    S.level = level;
    S.rb = rb;
    S.min_match = min_match;
    S.mbits = mbits;
    for (uint32_t k = 0; k < S.npieces; ++k) rf.push_back(zpq::UnlzWideRef{b, k});
    total_in += ((uint64_t)S.in_len + 3) & ~3ull;          // every start on a word
    slots += (uint64_t)S.npieces * piece;
  }
  const uint32_t np = (uint32_t)rf.size();
  uint8_t* in_all = emu::guard_alloc(total_in, 4, 0xA5);
  for (unsigned b = 0; b < nb; ++b) if (!in[b].empty()) memcpy(in_all + st[b].in_off, in[b].data(), in[b].size());
  Args a;
  memset(&a, 0, sizeof a);
  a.in_all = in_all;
  a.piece = piece;
  a.prov = (uint4*)emu::guard_alloc(16 * slots, 16, 0xEE);
  a.states = (uint32_t*)emu::guard_alloc(4 * slots, 4, 0xEE);
  a.fin = (uint4*)emu::guard_alloc(16 * slots, 16, 0xEE);
  a.pieces = (zpq::UnlzWidePieceOut*)emu::guard_alloc(sizeof(zpq::UnlzWidePieceOut) * np, 4, 0xEE);
  a.adopt = (zpq::UnlzWideAdopt*)emu::guard_alloc(sizeof(zpq::UnlzWideAdopt) * np, 4, 0);
  memset((void*)a.adopt, 0, sizeof(zpq::UnlzWideAdopt) * np);
  a.outs = (zpq::UnlzWideOut*)emu::guard_alloc(sizeof(zpq::UnlzWideOut) * nb, 8, 0xEE);
  zpq::UnlzWideStream* streams = (zpq::UnlzWideStream*)emu::guard_alloc(sizeof(zpq::UnlzWideStream) * nb, 8, 0);
  memcpy(streams, st.data(), sizeof(zpq::UnlzWideStream) * nb);
  zpq::UnlzWideRef* refs = (zpq::UnlzWideRef*)emu::guard_alloc(sizeof(zpq::UnlzWideRef) * np, 4, 0);
  if (np) memcpy(refs, rf.data(), sizeof(zpq::UnlzWideRef) * np);
  a.streams = streams;
  a.refs = refs;
  for (uint32_t g = 0; g < np; ++g) emu::run_workgroup(level == 1 ? piece_thunk<true> : piece_thunk<false>, &a, 64, g);
  for (unsigned b = 0; b < nb; ++b) emu::run_workgroup(level == 1 ? stitch_thunk<true> : stitch_thunk<false>, &a, 64, b);
  each_thread((uint64_t)np * ((piece + 255) / 256), [&] { zpq::unlzw_finalize_body(a.streams, a.refs, a.piece, a.prov, a.adopt, a.fin, a.outs); });
  // the host: the first failing token's status; the decoded, non-empty outputs packed (link, jump) and in their rooms (the filter)
  std::vector<uint32_t> status(nb), out_len(nb, 0);
  std::vector<uint64_t> room_off(nb, 0);
  std::vector<int> listed(nb, -1);                        // the stream's index in the filter's list
  std::vector<zpq::UnlzWidePlace> pl;
  std::vector<uint64_t> dst;
  std::vector<zpq::E8Block> bl;
  uint64_t packed = 0, placed = 0, tiles = 0;
  uint32_t sum[4] = {0, 0, 0, 0};
  for (unsigned b = 0; b < nb; ++b) {
    zpq::UnlzResult& r = a.outs[b].r;
    const zpq::UnlzWideStats& c = a.outs[b].stats;
    if (a.outs[b].err != ~0ull) r.status = (uint32_t)(a.outs[b].err & 7u);
    if (r.status == 0 && r.ntok > st[b].in_len) { fprintf(stderr, "stream %u: more tokens than stream bytes\n", b); return 3; }
    status[b] = r.status;
    sum[0] += c.pieces; sum[1] += c.entered; sum[2] += c.met; sum[3] += c.walked;
    if (r.status != 0 || !r.out_len) continue;
    out_len[b] = r.out_len;
    room_off[b] = placed;
    listed[b] = (int)bl.size();
    pl.push_back(zpq::UnlzWidePlace{packed, r.out_len, r.ntok, b, 0});
    dst.push_back(placed);
    bl.push_back(zpq::E8Block{placed, r.out_len, (uint32_t)tiles});
    packed += r.out_len;
    placed += zpq::e8_room(r.out_len);
    tiles += zpq::e8_tiles(r.out_len);
  }
  const uint32_t total = (uint32_t)packed, nlive = (uint32_t)pl.size();
  unsigned launches = 0;
  uint32_t rounds = 0;
  a.buf = emu::guard_alloc(placed, 16, 0xC3);
  const bool slack = placed && (placed % 4096) != 0;        // (guard_alloc: the buffer ends at the rear page; its page starts in front of it)
  if (slack) a.buf[-1] = 0x5A;
  if (total) {
    zpq::UnlzWidePlace* place = (zpq::UnlzWidePlace*)emu::guard_alloc(sizeof(zpq::UnlzWidePlace) * nlive, 8, 0);
    memcpy(place, pl.data(), sizeof(zpq::UnlzWidePlace) * nlive);
    uint64_t* dst_off = (uint64_t*)emu::guard_alloc(8 * (size_t)nlive, 8, 0);
    memcpy(dst_off, dst.data(), 8 * (size_t)nlive);
    uint32_t* w = (uint32_t*)emu::guard_alloc(4ull * total, 4, 0xEE);
    uint32_t* flags = (uint32_t*)emu::guard_alloc(4 * zpq::kUnlzWideRounds, 4, 0);
    memset(flags, 0, 4 * zpq::kUnlzWideRounds);
    const uint64_t blocks = ((uint64_t)total + 255) / 256;
    each_thread(blocks, [&] { zpq::unlzw_link_body(a.in_all, a.streams, place, nlive, total, a.fin, w); });
    ++launches;
    for (;;) {
      if (rounds == zpq::kUnlzWideRounds) { fprintf(stderr, "more than %u jump rounds\n", rounds); return 3; }
      uint32_t* const flag = flags + rounds++;
      each_thread(blocks, [&] { zpq::unlzw_jump_body(w, total, flag); });
      ++launches;
      if (!*flag) break;
    }
    each_thread(blocks, [&] { zpq::unlzw_emit_placed_body(w, place, dst_off, nlive, total, a.buf); });
    ++launches;
    // the filter over the rooms, as tests/emu/e8e9_emu_main.cpp runs it
    zpq::E8Block* blocks8 = (zpq::E8Block*)emu::guard_alloc(sizeof(zpq::E8Block) * bl.size(), 8, 0);
    memcpy(blocks8, bl.data(), sizeof(zpq::E8Block) * bl.size());
    a.blocks = blocks8;
    a.nblocks = (uint32_t)bl.size();
    a.ntiles = (uint32_t)tiles;
    a.max_steps = max_steps;
    a.cnt = (uint32_t*)emu::guard_alloc(4 * (2 * tiles + 1), 4, 0xEE);
    a.status = (uint32_t*)emu::guard_alloc(4 * bl.size(), 4, 0xEE);
    for (unsigned g = 0; g < tiles; ++g) emu::run_workgroup(mark_thunk, &a, 256, g);
    ++launches;
    uint32_t run = 0;                                             // the exclusive scan, in place
    for (uint64_t k = 0; k < 2 * tiles + 1; ++k) { const uint32_t c = a.cnt[k]; a.cnt[k] = run; run += c; }
    a.nseeds = a.cnt[tiles];
    const uint32_t nlist = a.cnt[2 * tiles];
    if (a.nseeds) {
      a.list = (uint32_t*)emu::guard_alloc(4 * (size_t)nlist, 4, 0xEE);
      for (unsigned g = 0; g < tiles; ++g) emu::run_workgroup(scatter_thunk, &a, 256, g);
      for (unsigned g = 0; g < (a.nseeds + 255u) / 256u; ++g) emu::run_workgroup(walk_thunk, &a, 256, g);
      launches += 2;
    }
    for (unsigned b = 0; b < nb; ++b)
      if (listed[b] >= 0 && a.status[listed[b]] != 0u) { status[b] = 1u; out_len[b] = 0; }      // a lane gave the block up
  }
  if (slack && a.buf[-1] != 0x5A) { fprintf(stderr, "the byte in front of the first room was written\n"); return 3; }
  for (unsigned b = 0; b < nb; ++b)
    printf("stream %u status %u out_len %u ntok %u listed %d\n", b, status[b], out_len[b], a.outs[b].r.ntok, listed[b] >= 0 ? 1 : 0);
  printf("pieces %u %u %u %u\n", sum[0], sum[1], sum[2], sum[3]);
  printf("rounds %u\n", rounds);
  printf("launches %u\n", launches);
  printf("edges ok\n");
  for (unsigned b = 0; b < nb; ++b) {
    if (status[b]) continue;
    const std::string path = prefix + "." + std::to_string(b);
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { perror(path.c_str()); return 2; }
    if (out_len[b]) fwrite(a.buf + room_off[b], 1, out_len[b], f);
    fclose(f);
  }
  return 0;
}
