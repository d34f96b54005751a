// TEST INFRASTRUCTURE -- LZ77 streams back into their blocks (zpaq_amd/csrc/device/lz77_decode_kernel.h) on the host-side
// wavefront emulator (wave_emu.h): unlz_parse_body, the host's placement of the outputs, then unlz_copy_body, for several
// streams in one batch as the engine lays them out.  Every array has its exact size between inaccessible pages (guard_alloc.h).
//
//   lz77_decode_emu <level> <rb> <min_match> <mbits> <out_prefix> <stream>[:<capacity>]...
//
// Prints "stream <k> status <s> out_len <n> ntok <t>" per stream.  When every stream with status 0 fits its capacity (if one is
// given), <out_prefix>.<k> = stream k's output for those; otherwise "overflow" and nothing is emitted, as in the engine.
#include "wave_emu.h"

#include <string>
#include <vector>

#include "guard_alloc.h"
#include "lz77_decode_kernel.h"

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
  const zpq::UnlzStream* streams;
  uint4* toks;
  zpq::UnlzResult* res;
  const uint64_t* out_off;
  uint8_t* out;
};

void parse_thunk(void* p) { Args* a = (Args*)p; zpq::unlz_parse_body(a->in_all, a->streams, a->toks, a->res); }
void copy_thunk(void* p) { Args* a = (Args*)p; zpq::unlz_copy_body(a->in_all, a->streams, a->toks, a->res, a->out_off, a->out); }

}  // namespace

int main(int argc, char** argv) {
  if (argc < 7) {
    fprintf(stderr, "usage: lz77_decode_emu <level> <rb> <min_match> <mbits> <out_prefix> <stream>[:<capacity>]...\n");
    return 2;
  }
  const uint32_t level = (uint32_t)atoi(argv[1]), rb = (uint32_t)atoi(argv[2]), min_match = (uint32_t)atoi(argv[3]), mbits = (uint32_t)atoi(argv[4]);
  const std::string prefix = argv[5];
  const unsigned nb = (unsigned)(argc - 6);
  std::vector<std::vector<uint8_t>> in(nb);
  std::vector<long long> cap(nb, -1);
  std::vector<zpq::UnlzStream> st(nb);
  uint64_t total = 0, ntok = 0;
  for (unsigned b = 0; b < nb; ++b) {
    std::string path = argv[6 + b];
    const size_t colon = path.rfind(':');
    if (colon != std::string::npos) { cap[b] = atoll(path.c_str() + colon + 1); path.resize(colon); }
    in[b] = slurp(path.c_str());
    zpq::UnlzStream& S = st[b];
    memset(&S, 0, sizeof S);
    S.in_off = total;
    S.tok_off = ntok;
    S.in_len = (uint32_t)in[b].size();
    S.tok_cap = S.in_len;
    S.level = level;
    S.rb = rb;
    S.min_match = min_match;
    S.mbits = mbits;
    total += ((uint64_t)S.in_len + 3) & ~3ull;          // every start on a word
    ntok += S.tok_cap;
  }
  uint8_t* in_all = emu::guard_alloc(total, 4, 0xA5);
  for (unsigned b = 0; b < nb; ++b) if (!in[b].empty()) memcpy(in_all + st[b].in_off, in[b].data(), in[b].size());
  uint4* toks = (uint4*)emu::guard_alloc(16 * ntok, 16, 0xEE);
  zpq::UnlzResult* res = (zpq::UnlzResult*)emu::guard_alloc(12 * nb, 4, 0xEE);
  zpq::UnlzStream* streams = (zpq::UnlzStream*)emu::guard_alloc(sizeof(zpq::UnlzStream) * nb, 8, 0);
  memcpy(streams, st.data(), sizeof(zpq::UnlzStream) * nb);
  Args a{in_all, streams, toks, res, nullptr, nullptr};
  for (unsigned b = 0; b < nb; ++b) emu::run_workgroup(parse_thunk, &a, 64, b);
  // the host: sizes first, then the outputs back to back, no byte between them
  bool fits = true;
  std::vector<uint64_t> off(nb + 1, 0);
  for (unsigned b = 0; b < nb; ++b) {
    printf("stream %u status %u out_len %u ntok %u\n", b, res[b].status, res[b].out_len, res[b].ntok);
    if (res[b].status == 0 && res[b].ntok > st[b].tok_cap) { fprintf(stderr, "stream %u: more tokens than slots\n", b); return 3; }
    const uint64_t len = res[b].status == 0 ? res[b].out_len : 0;
    if (cap[b] >= 0 && len > (uint64_t)cap[b]) fits = false;
    off[b + 1] = off[b] + len;
  }
  if (!fits) { printf("overflow\n"); return 0; }
  uint8_t* out = emu::guard_alloc(off[nb], 1, 0xC3);
  uint64_t* out_off = (uint64_t*)emu::guard_alloc(8 * nb, 8, 0);
  memcpy(out_off, off.data(), 8 * nb);
  a.out_off = out_off;
  a.out = out;
  for (unsigned b = 0; b < nb; ++b) emu::run_workgroup(copy_thunk, &a, 64, b);
  for (unsigned b = 0; b < nb; ++b) {
    if (res[b].status) continue;
    const std::string path = prefix + "." + std::to_string(b);
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { perror(path.c_str()); return 2; }
    fwrite(out + off[b], 1, off[b + 1] - off[b], f);
    fclose(f);
  }
  return 0;
}
