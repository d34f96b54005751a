// TEST INFRASTRUCTURE -- LZ77 streams back into their blocks, parsed in pieces (zpaq_amd/csrc/device/lz77_decode_wide_kernel.h),
// on the host-side wavefront emulator (wave_emu.h): the piece parse, the stitch, the finalize step, the host's placement of the
// outputs, then link, the jump rounds and emit, for several streams in one batch as the engine lays them out.  Every array has its
// exact size between inaccessible pages (guard_alloc.h).  The kernels of a lane per element have no cross-lane operation: their
// bodies run thread after thread, in the order ZPQ_EMU_ORDER says (reverse: the last thread of the last workgroup first).
//
//   lz77_decode_wide_emu <level> <rb> <min_match> <mbits> <piece> <out_prefix> <stream>[:<capacity>]...
//
// Prints "stream <k> status <s> out_len <n> ntok <t>" per stream and "pieces <all> <entered> <met> <walked>".  When every stream
// with status 0 fits its capacity (if one is given), "rounds <r>" and <out_prefix>.<k> = stream k's output for those; otherwise
// "overflow" and nothing is emitted, as in the engine.
#include "wave_emu.h"

#include <string>
#include <vector>

#include "guard_alloc.h"

// (fibers of one OS thread, switched only at cross-lane operations: a plain read-modify-write is atomic)
static inline unsigned long long atomicMin(unsigned long long* p, unsigned long long v) { const unsigned long long old = *p; if (v < old) *p = v; return old; }

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
  const zpq::UnlzWidePlace* place;
  uint32_t nlive, total;
  uint32_t* w;
  uint32_t* flag;
  uint8_t* out;
};

// (a batch is of one method: the kernels are instantiated for its level)
template <bool kBits>
void piece_thunk(void* p) { Args* a = (Args*)p; zpq::unlzw_piece_body<kBits>(a->in_all, a->streams, a->refs, a->piece, a->prov, a->states, a->pieces); }
template <bool kBits>
void stitch_thunk(void* p) {
  Args* a = (Args*)p;
  zpq::unlzw_stitch_body<kBits>(a->in_all, a->streams, a->piece, a->prov, a->states, a->pieces, a->fin, a->adopt, a->outs);
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
  if (argc < 8) {
    fprintf(stderr, "usage: lz77_decode_wide_emu <level> <rb> <min_match> <mbits> <piece> <out_prefix> <stream>[:<capacity>]...\n");
    return 2;
  }
  const uint32_t level = (uint32_t)atoi(argv[1]), rb = (uint32_t)atoi(argv[2]), min_match = (uint32_t)atoi(argv[3]), mbits = (uint32_t)atoi(argv[4]);
  const uint32_t piece = zpq::unlz_wide_piece_clamped((uint64_t)atoll(argv[5]));
  const std::string prefix = argv[6];
  const unsigned nb = (unsigned)(argc - 7);
  std::vector<std::vector<uint8_t>> in(nb);
  std::vector<long long> cap(nb, -1);
  std::vector<zpq::UnlzWideStream> st(nb);
  std::vector<zpq::UnlzWideRef> rf;
  uint64_t total_in = 0, slots = 0;
  for (unsigned b = 0; b < nb; ++b) {
    std::string path = argv[7 + b];
    const size_t colon = path.rfind(':');
    if (colon != std::string::npos) { cap[b] = atoll(path.c_str() + colon + 1); path.resize(colon); }
    in[b] = slurp(path.c_str());
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
  // the host: the first failing token's status, sizes first, then the outputs back to back, no byte between them
  bool fits = true;
  std::vector<uint64_t> off(nb + 1, 0);
  std::vector<zpq::UnlzWidePlace> pl;
  uint32_t sum[4] = {0, 0, 0, 0};
  for (unsigned b = 0; b < nb; ++b) {
    zpq::UnlzResult& r = a.outs[b].r;
    const zpq::UnlzWideStats& c = a.outs[b].stats;
    if (a.outs[b].err != ~0ull) r.status = (uint32_t)(a.outs[b].err & 7u);
    printf("stream %u status %u out_len %u ntok %u\n", b, r.status, r.out_len, r.ntok);
    if (r.status == 0 && r.ntok > st[b].in_len) { fprintf(stderr, "stream %u: more tokens than stream bytes\n", b); return 3; }
    const uint64_t len = r.status == 0 ? r.out_len : 0;
    if (cap[b] >= 0 && len > (uint64_t)cap[b]) fits = false;
    off[b + 1] = off[b] + len;
    if (len) pl.push_back(zpq::UnlzWidePlace{off[b], (uint32_t)len, r.ntok, b, 0});
    sum[0] += c.pieces; sum[1] += c.entered; sum[2] += c.met; sum[3] += c.walked;
  }
  printf("pieces %u %u %u %u\n", sum[0], sum[1], sum[2], sum[3]);
  if (!fits) { printf("overflow\n"); return 0; }
  const uint32_t total = (uint32_t)off[nb];
  zpq::UnlzWidePlace* place = (zpq::UnlzWidePlace*)emu::guard_alloc(sizeof(zpq::UnlzWidePlace) * pl.size(), 8, 0);
  if (!pl.empty()) memcpy(place, pl.data(), sizeof(zpq::UnlzWidePlace) * pl.size());
  a.place = place;
  a.nlive = (uint32_t)pl.size();
  a.total = total;
  a.w = (uint32_t*)emu::guard_alloc(4ull * total, 4, 0xEE);
  a.out = emu::guard_alloc(total, 1, 0xC3);
  a.flag = (uint32_t*)emu::guard_alloc(4 * zpq::kUnlzWideRounds, 4, 0);
  memset(a.flag, 0, 4 * zpq::kUnlzWideRounds);
  const uint64_t blocks = ((uint64_t)total + 255) / 256;
  each_thread(blocks, [&] { zpq::unlzw_link_body(a.in_all, a.streams, a.place, a.nlive, a.total, a.fin, a.w); });
  uint32_t rounds = 0;
  for (;;) {
    if (rounds == zpq::kUnlzWideRounds) { fprintf(stderr, "more than %u jump rounds\n", rounds); return 3; }
    uint32_t* const flag = a.flag + rounds++;
    each_thread(blocks, [&] { zpq::unlzw_jump_body(a.w, a.total, flag); });
    if (!*flag) break;
  }
  printf("rounds %u\n", rounds);
  each_thread(blocks, [&] { zpq::unlzw_emit_body(a.w, a.total, a.out); });
  for (unsigned b = 0; b < nb; ++b) {
    if (a.outs[b].r.status) continue;
    const std::string path = prefix + "." + std::to_string(b);
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { perror(path.c_str()); return 2; }
    fwrite(a.out + off[b], 1, off[b + 1] - off[b], f);
    fclose(f);
  }
  return 0;
}
