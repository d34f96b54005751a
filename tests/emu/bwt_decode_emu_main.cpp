// TEST INFRASTRUCTURE -- BWT streams back into their blocks (zpaq_amd/csrc/device/bwt_decode_kernel.h) on the host-side
// wavefront emulator (wave_emu.h): the host's admission of the streams and placement of the arrays as the engine does them,
// then the six kernels one after the other, for several streams in one batch.  Every array has its exact size between
// inaccessible pages (guard_alloc.h) and starts dirty.
//
//   bwt_decode_emu run <mbits> <out_prefix> <stream>[:<capacity>]...
//   bwt_decode_emu admit <mbits> <out_prefix> <stream>...        the host's step alone: no kernel runs
//
// Prints "stream <k> status <s> out_len <n>" per stream (admit: status 0 for a stream the kernels would be given).  When every
// admitted stream fits its capacity (if one is given), <out_prefix>.<k> = stream k's output for those with status 0; otherwise
// "overflow", every size as the host knows it, and nothing runs, as in the engine.
#include "wave_emu.h"

#include <string>
#include <vector>

// a workgroup's fibers run on one OS thread and switch only at cross-lane operations and barriers, so a plain
// read-modify-write is atomic
static inline unsigned atomicAdd(unsigned* p, unsigned v) { const unsigned old = *p; *p = old + v; return old; }

#include "bwt_decode_kernel.h"
#include "guard_alloc.h"

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
  const zpq::BwtStream* streams;
  uint32_t nstreams, nsplit;
  uint32_t* hist;
  uint32_t* link;
  uint4* sp;
  uint32_t* status;
  uint8_t* out;
};

void count_thunk(void* p) { Args* a = (Args*)p; zpq::unbwt_count_body(a->in_all, a->streams, a->nstreams, a->hist); }
void scan_thunk(void* p) { Args* a = (Args*)p; zpq::unbwt_scan_body(a->streams, a->hist); }
void link_thunk(void* p) { Args* a = (Args*)p; zpq::unbwt_link_body(a->in_all, a->streams, a->nstreams, a->hist, a->link); }
void rank_thunk(void* p) { Args* a = (Args*)p; zpq::unbwt_rank_body(a->streams, a->nstreams, a->nsplit, a->link, a->sp); }
void offsets_thunk(void* p) { Args* a = (Args*)p; zpq::unbwt_offsets_body(a->streams, a->sp, a->status); }
void emit_thunk(void* p) { Args* a = (Args*)p; zpq::unbwt_emit_body(a->streams, a->nstreams, a->nsplit, a->link, a->sp, a->status, a->out); }

}  // namespace

int main(int argc, char** argv) {
  if (argc < 5 || (strcmp(argv[1], "run") && strcmp(argv[1], "admit"))) {
    fprintf(stderr, "usage: bwt_decode_emu run|admit <mbits> <out_prefix> <stream>[:<capacity>]...\n");
    return 2;
  }
  const bool admit_only = !strcmp(argv[1], "admit");
  const uint32_t mbits = (uint32_t)atoi(argv[2]);
  const std::string prefix = argv[3];
  const unsigned nb = (unsigned)(argc - 4);
  std::vector<std::vector<uint8_t>> in(nb);
  std::vector<long long> cap(nb, -1);
  std::vector<int> slot(nb, -1);                      // the stream's place among the admitted ones; -2: the empty block
  std::vector<zpq::BwtStream> st;
  uint64_t in_bytes = 0, nodes = 0, tiles = 0, splits = 0, room = 0;
  bool fits = true;
  for (unsigned b = 0; b < nb; ++b) {
    std::string path = argv[4 + b];
    const size_t colon = path.rfind(':');
    if (colon != std::string::npos) { cap[b] = atoll(path.c_str() + colon + 1); path.resize(colon); }
    in[b] = slurp(path.c_str());
    if (zpq::bwt_stream_empty(in[b].data(), in[b].size())) { slot[b] = -2; continue; }
    zpq::BwtStream S;
    memset(&S, 0, sizeof S);
    if (!zpq::bwt_stream_admitted(in[b].data(), in[b].size(), mbits, S.n, S.idx)) continue;
    S.in_off = in_bytes;
    S.link_off = nodes;
    S.out_off = room;
    S.tile_off = (uint32_t)tiles;
    S.sp_off = (uint32_t)splits;
    in_bytes += ((uint64_t)in[b].size() + 3) & ~3ull;          // every start on a word
    nodes += (uint64_t)S.n + 1;
    tiles += zpq::bwt_tiles(S.n);
    splits += zpq::bwt_splitters(S.n);
    room += S.n;                                               // the outputs back to back, no byte between them
    if (cap[b] >= 0 && (long long)S.n > cap[b]) fits = false;
    slot[b] = (int)st.size();
    st.push_back(S);
  }
  const unsigned m = (unsigned)st.size();
  if (admit_only || !fits) {
    for (unsigned b = 0; b < nb; ++b) printf("stream %u status %d out_len %u\n", b, slot[b] == -1 ? 1 : 0, slot[b] >= 0 ? st[slot[b]].n : 0u);
    if (!fits) printf("overflow\n");
    return 0;
  }
  std::vector<uint32_t> status_host(m, 1);
  uint8_t* out = nullptr;
  if (m) {
    uint8_t* in_all = emu::guard_alloc(in_bytes, 4, 0xA5);
    for (unsigned b = 0; b < nb; ++b) if (slot[b] >= 0) memcpy(in_all + st[slot[b]].in_off, in[b].data(), in[b].size());
    zpq::BwtStream* streams = (zpq::BwtStream*)emu::guard_alloc(sizeof(zpq::BwtStream) * m, 8, 0);
    memcpy(streams, st.data(), sizeof(zpq::BwtStream) * m);
    Args a;
    a.in_all = in_all;
    a.streams = streams;
    a.nstreams = m;
    a.nsplit = (uint32_t)splits;
    a.hist = (uint32_t*)emu::guard_alloc(1024 * tiles, 4, 0xEE);
    a.link = (uint32_t*)emu::guard_alloc(4 * nodes, 4, 0xEE);
    a.sp = (uint4*)emu::guard_alloc(16 * splits, 16, 0xEE);
    a.status = (uint32_t*)emu::guard_alloc(4 * m, 4, 0xEE);
    a.out = out = emu::guard_alloc(room, 1, 0xC3);
    const unsigned spb = ((unsigned)splits + 255u) / 256u;
    for (unsigned g = 0; g < tiles; ++g) emu::run_workgroup(count_thunk, &a, 64, g);
    for (unsigned b = 0; b < m; ++b) emu::run_workgroup(scan_thunk, &a, 256, b);
    for (unsigned g = 0; g < tiles; ++g) emu::run_workgroup(link_thunk, &a, 64, g);
    for (unsigned g = 0; g < spb; ++g) emu::run_workgroup(rank_thunk, &a, 256, g);
    for (unsigned b = 0; b < m; ++b) emu::run_workgroup(offsets_thunk, &a, 64, b);
    for (unsigned g = 0; g < spb; ++g) emu::run_workgroup(emit_thunk, &a, 256, g);
    for (unsigned k = 0; k < m; ++k) status_host[k] = a.status[k];
    // a declined stream's part of the output is as it was
    for (unsigned k = 0; k < m; ++k)
      if (status_host[k])
        for (uint64_t q = 0; q < st[k].n; ++q)
          if (out[st[k].out_off + q] != 0xC3) { fprintf(stderr, "stream slot %u: declined, but its output was written\n", k); return 3; }
  }
  for (unsigned b = 0; b < nb; ++b) {
    const bool ok = slot[b] == -2 || (slot[b] >= 0 && status_host[slot[b]] == 0);
    printf("stream %u status %d out_len %u\n", b, ok ? 0 : 1, ok && slot[b] >= 0 ? st[slot[b]].n : 0u);
    if (!ok) continue;
    const std::string path = prefix + "." + std::to_string(b);
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { perror(path.c_str()); return 2; }
    if (slot[b] >= 0) fwrite(out + st[slot[b]].out_off, 1, st[slot[b]].n, f);
    fclose(f);
  }
  return 0;
}
