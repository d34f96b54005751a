// TEST INFRASTRUCTURE -- the device's generic post-processor on the host-side wavefront emulator (wave_emu.h): the text
// zpq_pcomp_source generates for one PCOMP program (zpaq_amd/csrc/device/pcomp_kernel.h with pcomp_body, and the program
// translated by host/codegen.cpp) is compiled into this executable in front of this file.  One launch as engine_pcomp makes
// it: a job per stream, a workgroup of 64 lanes per 64 jobs, every lane's M (2^pm bytes), H (2^ph words), R (256 words), input
// and output (out_cap bytes) at their exact sizes between inaccessible pages (guard_alloc.h) -- M, H and R zeroed as the engine
// zeroes them, the output dirty -- and the job and result arrays likewise.
//
//   pcomp_emu run <ph> <pm> <spec> <input> <output>
//
// <spec>: one line "<in_len> <out_cap>" per stream; <input>: the streams back to back.  Prints "stream <k> n <result[0]> status
// <result[1]>" per stream; <output>: min(result[0], out_cap) bytes of every stream's buffer, back to back.
#include "wave_emu.h"

#include <string>
#include <vector>

#include "guard_alloc.h"
#include "layout.h"

extern "C" void zpq_pcomp_run(const zpq::PcompJob* jobs, unsigned n);

namespace {

struct Args { const zpq::PcompJob* jobs; unsigned n; };
void thunk(void* p) { Args* a = (Args*)p; zpq_pcomp_run(a->jobs, a->n); }

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

}  // namespace

int main(int argc, char** argv) {
  if (argc != 7 || strcmp(argv[1], "run")) {
    fprintf(stderr, "usage: pcomp_emu run <ph> <pm> <spec> <input> <output>\n");
    return 2;
  }
  const int ph = atoi(argv[2]), pm = atoi(argv[3]);
  if (ph < 0 || ph > 24 || pm < 0 || pm > 26) { fprintf(stderr, "pcomp_emu: arrays too large for a test\n"); return 2; }
  std::vector<unsigned long long> in_len, cap;
  {
    FILE* f = fopen(argv[4], "r");
    if (!f) { perror(argv[4]); return 2; }
    unsigned long long a, b;
    while (fscanf(f, "%llu %llu", &a, &b) == 2) { in_len.push_back(a); cap.push_back(b); }
    fclose(f);
  }
  const std::vector<uint8_t> input = slurp(argv[5]);
  const unsigned n = (unsigned)in_len.size();
  unsigned long long total = 0;
  for (unsigned i = 0; i < n; ++i) {
    if (cap[i] > 0xFFFFFFF0ull) { fprintf(stderr, "pcomp_emu: a capacity the engine never launches\n"); return 2; }
    total += in_len[i];
  }
  if (!n || total != input.size()) { fprintf(stderr, "pcomp_emu: spec and input disagree\n"); return 2; }
  zpq::PcompJob* jobs = (zpq::PcompJob*)emu::guard_alloc(sizeof(zpq::PcompJob) * n, 8, 0);
  uint32_t* results = (uint32_t*)emu::guard_alloc(8 * (size_t)n, 4, 0xEE);
  size_t at = 0;
  for (unsigned i = 0; i < n; ++i) {
    zpq::PcompJob& j = jobs[i];
    uint8_t* in = emu::guard_alloc(in_len[i], 1, 0x5A);
    if (in_len[i]) memcpy(in, input.data() + at, in_len[i]);
    at += in_len[i];
    j.in = in;
    j.out = emu::guard_alloc(cap[i], 1, 0xA5);
    j.M = emu::guard_alloc((size_t)1 << pm, 1, 0);
    j.H = (uint32_t*)emu::guard_alloc((size_t)4 << ph, 4, 0);
    j.R = (uint32_t*)emu::guard_alloc(1024, 4, 0);
    j.in_len = (uint32_t)in_len[i];
    j.out_cap = (uint32_t)cap[i];
    j.result = results + 2 * i;
  }
  Args a{jobs, n};
  for (unsigned g = 0; g < (n + 63) / 64; ++g) emu::run_workgroup(thunk, &a, 64, g);
  FILE* f = fopen(argv[6], "wb");
  if (!f) { perror(argv[6]); return 2; }
  for (unsigned i = 0; i < n; ++i) {
    printf("stream %u n %u status %u\n", i, results[2 * i], results[2 * i + 1]);
    const size_t w = results[2 * i] < cap[i] ? results[2 * i] : (size_t)cap[i];
    if (w) fwrite(jobs[i].out, 1, w, f);
  }
  fclose(f);
  return 0;
}
