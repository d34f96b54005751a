// TEST INFRASTRUCTURE -- the driver of both BWT decoders (zpaq_amd/csrc/device/bwt_decode_kernel.h and
// bwt_decode_wide_kernel.h) on the host-side wavefront emulator (wave_emu.h): the host's admission of the streams, the cut into
// sub-batches (the wide form's) and the placement of the arrays as the engine does them (layout.h bwt_stream_admitted /
// bwt_wide_stream_admitted, bwt_wide_cut, BwtNeed), then the form's kernels one after the other per sub-batch.  Every array has
// its exact size between inaccessible pages (guard_alloc.h) and starts dirty.  bwt_decode_emu_main.cpp and
// bwt_decode_wide_emu_main.cpp are this body at the two widths of a node:
//
//   <exe> run <mbits> <out_limit> <out_prefix> <stream>[:<capacity>]...
//   <exe> admit <mbits> <out_limit> <out_prefix> <stream>...        the host's step alone: no kernel runs
//   <exe> range <mbits> <n>                                         the admission of a stream of n zeros with idx 1 (S[1] = 255)
//                                                                   that is never built: "admitted 0|1 small 0|1 n <n>"
//
// out_limit: the bytes of output a sub-batch of the wide form may hold (0: the engine's 2 GiB) -- the limit the engine cuts a
// batch by, injected; the small form is one batch whatever it says, as in the engine.  Prints "stream <k> status <s> out_len <n>"
// per stream (admit: status 0 for a stream the kernels would be given) and "batches <b>", the sub-batches that ran.  When every
// admitted stream fits its capacity (if one is given), <out_prefix>.<k> = stream k's output for those with status 0; otherwise
// "overflow", every size as the host knows it, and nothing runs, as in the engine.
#pragma once
#include "wave_emu.h"

#include <string>
#include <type_traits>
#include <vector>

// a workgroup's fibers run on one OS thread and switch only at cross-lane operations and barriers, so a plain
// read-modify-write is atomic
static inline unsigned atomicAdd(unsigned* p, unsigned v) { const unsigned old = *p; *p = old + v; return old; }

#include "bwt_decode_wide_kernel.h"
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

template <bool Wide>
struct BwtEmu {
  typedef typename std::conditional<Wide, uint64_t, uint32_t>::type Word;      // a node of the list
  struct Args {
    const uint8_t* in_all;
    const zpq::BwtStream* streams;
    const uint32_t* sp2_off;
    uint32_t nstreams, nsplit, nsplit2;
    uint32_t* hist;
    Word* link;
    uint4* sp;
    uint4* sp2;
    uint32_t* status;
    uint8_t* out;
  };
  static void count_thunk(void* p) { Args* a = (Args*)p; zpq::unbwt_count_body(a->in_all, a->streams, a->nstreams, a->hist); }
  static void scan_thunk(void* p) {
    Args* a = (Args*)p;
    if (Wide) zpq::unbwt_wide_scan_body(a->streams, a->hist);
    else zpq::unbwt_scan_body(a->streams, a->hist);
  }
  static void link_thunk(void* p) { Args* a = (Args*)p; zpq::unbwt_link_body(a->in_all, a->streams, a->nstreams, a->hist, a->link); }
  static void rank_thunk(void* p) { Args* a = (Args*)p; zpq::unbwt_rank_body(a->streams, a->nstreams, a->nsplit, a->link, a->sp); }
  static void offsets_thunk(void* p) { Args* a = (Args*)p; zpq::unbwt_offsets_body(a->streams, a->sp, a->status); }
  static void rank2_thunk(void* p) { Args* a = (Args*)p; zpq::unbwt_wide_rank2_body(a->streams, a->sp2_off, a->nstreams, a->nsplit2, a->sp, a->sp2); }
  static void offsets2_thunk(void* p) { Args* a = (Args*)p; zpq::unbwt_wide_offsets2_body(a->streams, a->sp2_off, a->sp2, a->status); }
  static void offsets1_thunk(void* p) {
    Args* a = (Args*)p;
    zpq::unbwt_wide_offsets1_body(a->streams, a->sp2_off, a->nstreams, a->nsplit2, a->sp, a->sp2, a->status);
  }
  static void emit_thunk(void* p) { Args* a = (Args*)p; zpq::unbwt_emit_body(a->streams, a->nstreams, a->nsplit, a->link, a->sp, a->status, a->out); }

  // the form's stages over one placed batch, in the order of launch_bwt_decode / launch_bwt_decode_wide
  static void stages(Args& a, const zpq::BwtNeed& w) {
    const unsigned m = a.nstreams, spb = ((unsigned)w.splits + 255u) / 256u, spb2 = ((unsigned)w.splits2 + 255u) / 256u;
    for (unsigned g = 0; g < w.tiles; ++g) emu::run_workgroup(count_thunk, &a, 64, g);
    for (unsigned b = 0; b < m; ++b) emu::run_workgroup(scan_thunk, &a, Wide ? 256 * zpq::kBwtScanParts : 256, b);
    for (unsigned g = 0; g < w.tiles; ++g) emu::run_workgroup(link_thunk, &a, 64, g);
    for (unsigned g = 0; g < spb; ++g) emu::run_workgroup(rank_thunk, &a, 256, g);
    if (Wide) {
      for (unsigned g = 0; g < spb2; ++g) emu::run_workgroup(rank2_thunk, &a, 256, g);
      for (unsigned b = 0; b < m; ++b) emu::run_workgroup(offsets2_thunk, &a, 64, b);
      for (unsigned g = 0; g < spb2; ++g) emu::run_workgroup(offsets1_thunk, &a, 256, g);
    } else {
      for (unsigned b = 0; b < m; ++b) emu::run_workgroup(offsets_thunk, &a, 64, b);
    }
    for (unsigned g = 0; g < spb; ++g) emu::run_workgroup(emit_thunk, &a, 256, g);
  }

  static int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "range")) {
      // the admission reads S[idx] and the four bytes of idx only: a sparse view of the stream serves
      const uint32_t mbits = (uint32_t)atoi(argv[2]);
      const uint64_t n = strtoull(argv[3], nullptr, 10);
      uint8_t* s = (uint8_t*)calloc(n + 5, 1);            // (untouched pages cost nothing)
      if (!s) { perror("calloc"); return 2; }
      s[1] = 255;
      s[n + 1] = 1;
      uint32_t sn = 0, sidx = 0;
      const bool ok = zpq::bwt_wide_stream_admitted(s, n + 5, mbits, sn, sidx);
      uint32_t tn = 0, tidx = 0;
      const bool small = zpq::bwt_stream_admitted(s, n + 5, mbits, tn, tidx);
      printf("admitted %d small %d n %u\n", ok ? 1 : 0, small ? 1 : 0, ok ? sn : 0u);
      return 0;
    }
    if (argc < 6 || (strcmp(argv[1], "run") && strcmp(argv[1], "admit"))) {
      fprintf(stderr, "usage: %s run|admit <mbits> <out_limit> <out_prefix> <stream>[:<capacity>]...\n", argv[0]);
      return 2;
    }
    const bool admit_only = !strcmp(argv[1], "admit");
    const uint32_t mbits = (uint32_t)atoi(argv[2]);
    const uint64_t out_limit = strtoull(argv[3], nullptr, 10) ? strtoull(argv[3], nullptr, 10) : 1ull << 31;
    const std::string prefix = argv[4];
    const unsigned nb = (unsigned)(argc - 5);
    std::vector<std::vector<uint8_t>> in(nb);
    std::vector<long long> cap(nb, -1);
    std::vector<int> slot(nb, -1);                      // the stream's place among the admitted ones; -2: the empty block
    std::vector<uint32_t> ns, idxs;
    std::vector<unsigned> who;
    bool fits = true;
    for (unsigned b = 0; b < nb; ++b) {
      std::string path = argv[5 + b];
      const size_t colon = path.rfind(':');
      if (colon != std::string::npos) { cap[b] = atoll(path.c_str() + colon + 1); path.resize(colon); }
      in[b] = slurp(path.c_str());
      if (zpq::bwt_stream_empty(in[b].data(), in[b].size())) { slot[b] = -2; continue; }
      uint32_t sn = 0, sidx = 0;
      if (!(Wide ? zpq::bwt_wide_stream_admitted(in[b].data(), in[b].size(), mbits, sn, sidx)
                 : zpq::bwt_stream_admitted(in[b].data(), in[b].size(), mbits, sn, sidx)))
        continue;
      if (cap[b] >= 0 && (long long)sn > cap[b]) fits = false;
      slot[b] = (int)ns.size();
      ns.push_back(sn);
      idxs.push_back(sidx);
      who.push_back(b);
    }
    const size_t m = ns.size();
    if (admit_only || !fits) {
      for (unsigned b = 0; b < nb; ++b) printf("stream %u status %d out_len %u\n", b, slot[b] == -1 ? 1 : 0, slot[b] >= 0 ? ns[slot[b]] : 0u);
      if (!fits) printf("overflow\n");
      return 0;
    }
    std::vector<uint32_t> status_host(m, 1);
    std::vector<std::vector<uint8_t>> result(m);
    unsigned batches = 0;
    for (size_t from = 0; from < m;) {
      const size_t end = Wide ? zpq::bwt_wide_cut(ns.data(), m, from, out_limit, ~0ull, false) : m;
      if (end == from) { ++from; continue; }            // does not fit alone: declined
      ++batches;
      const unsigned mm = (unsigned)(end - from);
      std::vector<zpq::BwtStream> st(mm);
      std::vector<uint32_t> s2(mm);
      zpq::BwtNeed w;
      for (unsigned k = 0; k < mm; ++k) st[k] = w.place(ns[from + k], idxs[from + k], false, &s2[k]);
      uint8_t* in_all = emu::guard_alloc(w.in_bytes, 4, 0xA5);
      for (unsigned k = 0; k < mm; ++k) memcpy(in_all + st[k].in_off, in[who[from + k]].data(), in[who[from + k]].size());
      zpq::BwtStream* streams = (zpq::BwtStream*)emu::guard_alloc(sizeof(zpq::BwtStream) * mm, 8, 0);
      memcpy(streams, st.data(), sizeof(zpq::BwtStream) * mm);
      Args a;
      a.in_all = in_all;
      a.streams = streams;
      a.sp2_off = nullptr;
      a.nstreams = mm;
      a.nsplit = (uint32_t)w.splits;
      a.nsplit2 = (uint32_t)w.splits2;
      a.hist = (uint32_t*)emu::guard_alloc(1024 * w.tiles, 4, 0xEE);
      a.link = (Word*)emu::guard_alloc(sizeof(Word) * w.nodes, sizeof(Word), 0xEE);
      a.sp = (uint4*)emu::guard_alloc(16 * w.splits, 16, 0xEE);
      a.sp2 = nullptr;
      if (Wide) {                                       // the second level's tables: the small form has none
        uint32_t* sp2_off = (uint32_t*)emu::guard_alloc(4 * mm, 4, 0);
        memcpy(sp2_off, s2.data(), 4 * mm);
        a.sp2_off = sp2_off;
        a.sp2 = (uint4*)emu::guard_alloc(16 * w.splits2, 16, 0xEE);
      }
      a.status = (uint32_t*)emu::guard_alloc(4 * mm, 4, 0xEE);
      a.out = emu::guard_alloc(w.room, 1, 0xC3);
      stages(a, w);
      for (unsigned k = 0; k < mm; ++k) {
        status_host[from + k] = a.status[k];
        if (a.status[k]) {                              // a declined stream's part of the output is as it was
          for (uint64_t q = 0; q < st[k].n; ++q)
            if (a.out[st[k].out_off + q] != 0xC3) { fprintf(stderr, "stream slot %zu: declined, but its output was written\n", from + k); return 3; }
        } else {
          result[from + k].assign(a.out + st[k].out_off, a.out + st[k].out_off + st[k].n);
        }
      }
      from = end;
    }
    for (unsigned b = 0; b < nb; ++b) {
      const bool ok = slot[b] == -2 || (slot[b] >= 0 && status_host[slot[b]] == 0);
      printf("stream %u status %d out_len %u\n", b, ok ? 0 : 1, ok && slot[b] >= 0 ? ns[slot[b]] : 0u);
      if (!ok) continue;
      const std::string path = prefix + "." + std::to_string(b);
      FILE* f = fopen(path.c_str(), "wb");
      if (!f) { perror(path.c_str()); return 2; }
      if (slot[b] >= 0) fwrite(result[slot[b]].data(), 1, result[slot[b]].size(), f);
      fclose(f);
    }
    printf("batches %u\n", batches);
    return 0;
  }
};

}  // namespace
