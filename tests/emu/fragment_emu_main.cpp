// TEST INFRASTRUCTURE -- fragmenting on the device (zpaq_amd/csrc/device/fragment_kernel.h and the host's stitch,
// device/fragment_stitch.hpp) on the host-side wavefront emulator (wave_emu.h): the files placed as the engine places them, the
// pieces, round 0 and the fix-up rounds, a workgroup of 64 per job.  Every array has its exact size between inaccessible pages
// (guard_alloc.h) and starts dirty; the job and result arrays are made anew for every launch.
//
//   fragment_emu run <piece> <min> <max> <thresh> <out> <file>...
//
// Prints "rounds <r>" and "file <k> fragments <n>" per file; <out> = the files' records back to back (264 bytes each: end, hits,
// the table).
#include "wave_emu.h"

#include <string>
#include <vector>

#include "fragment_kernel.h"
#include "fragment_stitch.hpp"
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
  const uint8_t* buf;
  const zpq::FragJob* jobs;
  uint32_t njobs;
  zpq::FragParams P;
  zpq::FragRec* recs;
  zpq::FragResult* res;
};
void walk_thunk(void* p) { Args* a = (Args*)p; zpq::frag_walk_body(a->buf, a->jobs, a->njobs, a->P, a->recs, a->res); }

}  // namespace

int main(int argc, char** argv) {
  if (argc < 8 || strcmp(argv[1], "run")) {
    fprintf(stderr, "usage: fragment_emu run <piece> <min> <max> <thresh> <out> <file>...\n");
    return 2;
  }
  const uint64_t piece = strtoull(argv[2], nullptr, 10);
  Args a;
  a.P.min_frag = (uint32_t)strtoul(argv[3], nullptr, 10);
  a.P.max_frag = (uint32_t)strtoul(argv[4], nullptr, 10);
  a.P.thresh = (uint32_t)strtoul(argv[5], nullptr, 10);
  const char* outpath = argv[6];
  const uint32_t n = (uint32_t)(argc - 7);
  std::vector<std::vector<uint8_t>> in(n);
  std::vector<uint64_t> off(n), len(n);
  uint64_t bytes = 0;
  for (uint32_t f = 0; f < n; ++f) {
    in[f] = slurp(argv[7 + f]);
    len[f] = in[f].size();
    off[f] = bytes;
    bytes += f + 1 < n ? (len[f] + 63) & ~63ull : len[f];        // (the last file ends where the buffer ends)
  }
  zpq::FragPlan pl;
  if (piece < 64 || !zpq::frag_plan(len.data(), n, piece, a.P.min_frag, pl)) { fprintf(stderr, "plan failed\n"); return 2; }
  uint8_t* buf = emu::guard_alloc(bytes, 1, 0xA5);
  for (uint32_t f = 0; f < n; ++f) if (len[f]) memcpy(buf + off[f], in[f].data(), len[f]);
  a.buf = buf;
  a.recs = (zpq::FragRec*)emu::guard_alloc(sizeof(zpq::FragRec) * pl.nrec * (pl.pieces ? 2 : 1), 8, 0xEE);
  auto run = [&](const std::vector<zpq::FragJob>& jb, std::vector<zpq::FragResult>& rs, std::vector<std::vector<zpq::FragRec>>& lists) -> bool {
    const size_t q = jb.size();
    zpq::FragJob* dj = (zpq::FragJob*)emu::guard_alloc(sizeof(zpq::FragJob) * q, 8, 0xEE);
    memcpy(dj, jb.data(), sizeof(zpq::FragJob) * q);
    a.jobs = dj;
    a.njobs = (uint32_t)q;
    a.res = (zpq::FragResult*)emu::guard_alloc(sizeof(zpq::FragResult) * q, 4, 0xEE);
    for (size_t g = 0; g < q; ++g) emu::run_workgroup(walk_thunk, &a, 64, (unsigned)g);
    rs.assign(a.res, a.res + q);
    if (!zpq::frag_results_ok(jb, rs)) { fprintf(stderr, "a record list overflowed\n"); return false; }
    lists.assign(q, std::vector<zpq::FragRec>());
    for (size_t g = 0; g < q; ++g) lists[g].assign(a.recs + jb[g].rec_off, a.recs + jb[g].rec_off + rs[g].count);
    return true;
  };
  std::vector<std::vector<zpq::FragRec>> fin;
  uint32_t rounds = 0;
  std::string note;
  if (!zpq::frag_stitch(pl, off.data(), len.data(), n, piece, run, fin, rounds, note)) { fprintf(stderr, "stitch failed: %s\n", note.c_str()); return 3; }
  FILE* o = fopen(outpath, "wb");
  if (!o) { perror(outpath); return 2; }
  printf("rounds %u\n", rounds);
  for (uint32_t f = 0; f < n; ++f) {
    printf("file %u fragments %zu\n", f, fin[f].size());
    if (!fin[f].empty()) fwrite(fin[f].data(), sizeof(zpq::FragRec), fin[f].size(), o);
  }
  fclose(o);
  return 0;
}
