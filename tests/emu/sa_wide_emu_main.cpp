// TEST INFRASTRUCTURE -- the wide suffix sort (zpaq_amd/csrc/device/sa_wide_kernel.h, the loop of build_suffix_array_wide in
// device/sa_kernels.hip) on the host-side wavefront emulator: the kernel bodies and the host helpers of that very file in the
// order the loop runs them, 256 threads per workgroup.  The two library calls have stand-ins, as in sa_emu.h: the radix sort is
// std::stable_sort on the key MASKED to the 2 w bits the sort is asked for (a field too narrow for its ranks loses their top
// bits; so does this), the scan is std::partial_sum.  Every array has its exact size -- n elements, not the engine's round-up
// to 64 -- ends at an inaccessible page (guard_alloc.h) and is dirty (0xA5) at the start.
//
//   sa_wide_emu sort <rank_bits> <out_prefix> <input>...
//       every input is one block, sorted alone.  rank_bits 0: sa_wide_rank_bits(n); else the forced field width.  Block k:
//       <out_prefix>.<k>.sa = the suffix array, .rank = the ranks the loop ends with (little-endian uint32 each), .bwt = the
//       stream bwt_wide_body's column and index make (n + 5 bytes); one line "block <k> n <n> bits <r> rounds <rounds>" each.
//   sa_wide_emu bits <n>                           sa_wide_rank_bits(n)                        -> "bits <r>"
//   sa_wide_emu field <r> <h>                      sa_wide_field_bits(r, h)                    -> "field <w>"
#include "wave_emu.h"

#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "guard_alloc.h"
#include "sa_wide_kernel.h"

namespace {

template <class T>
T* guarded(size_t n) { return (T*)emu::guard_alloc(n * sizeof(T), alignof(T), 0xA5); }

struct Args {
  const uint8_t* in;
  uint32_t n, h, w;
  uint32_t* rank;
  uint64_t *keys, *keys2;
  uint32_t *vals, *vals2, *flags, *sa;
  uint8_t* bwt;
  uint32_t* idx;
};

void init_thunk(void* p) { Args* a = (Args*)p; zpq::sa_wide_init_body(a->in, a->n, a->rank); }
void keys_thunk(void* p) { Args* a = (Args*)p; zpq::sa_wide_keys_body(a->rank, a->n, a->h, a->w, a->keys, a->vals); }
void flags_thunk(void* p) { Args* a = (Args*)p; zpq::sa_flags_body(a->keys2, a->n, a->flags); }
void rename_thunk(void* p) { Args* a = (Args*)p; zpq::sa_wide_rename_body(a->vals2, a->flags, a->n, a->rank); }
void invert_thunk(void* p) { Args* a = (Args*)p; zpq::sa_wide_invert_body(a->rank, a->n, a->sa); }
void bwt_thunk(void* p) { Args* a = (Args*)p; zpq::bwt_wide_body(a->in, a->rank, a->n, a->bwt, a->idx); }

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

void dump(const std::string& path, const void* p, size_t bytes) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) { perror(path.c_str()); exit(2); }
  if (bytes) fwrite(p, 1, bytes, f);
  fclose(f);
}

int usage() {
  fprintf(stderr, "usage: sa_wide_emu sort <rank_bits> <out_prefix> <input>... | bits <n> | field <r> <h>\n");
  return 2;
}

// build_suffix_array_wide and launch_bwt_wide for one block; exits with 2 for a block they refuse, with 3 when the loop does not end
void sort_block(unsigned k, const std::vector<uint8_t>& input, unsigned rank_bits, const std::string& prefix) {
  const std::string base = prefix + "." + std::to_string(k);
  const uint64_t n64 = input.size();
  if (!n64) { fprintf(stderr, "an empty block never reaches the sorter\n"); exit(2); }
  const unsigned r = rank_bits ? rank_bits : zpq::sa_wide_rank_bits(n64);
  if (n64 >= (1ull << 31) || r > 32 || r < zpq::sa_wide_rank_bits(n64)) { fprintf(stderr, "block outside the sorter's range\n"); exit(2); }
  const uint32_t n = (uint32_t)n64;
  uint8_t* in = guarded<uint8_t>(n);
  memcpy(in, input.data(), n);
  Args a{in, n, 1, 0, guarded<uint32_t>(n), guarded<uint64_t>(n), guarded<uint64_t>(n), guarded<uint32_t>(n), guarded<uint32_t>(n),
         guarded<uint32_t>(n), guarded<uint32_t>(n), guarded<uint8_t>((size_t)n + 1), guarded<uint32_t>(1)};
  const unsigned g = (unsigned)(((uint64_t)n + 255) / 256);
  auto launch = [&](emu::KernelFn fn) { for (unsigned wg = 0; wg < g; ++wg) emu::run_workgroup(fn, &a, 256, wg); };
  launch(init_thunk);
  std::vector<uint32_t> perm(n);
  uint32_t rounds = 0;
  for (;; a.h <<= 1) {
    a.w = zpq::sa_wide_field_bits(r, a.h);
    launch(keys_thunk);
    const uint64_t mask = 2 * a.w >= 64 ? ~0ull : (1ull << (2 * a.w)) - 1;
    std::iota(perm.begin(), perm.end(), 0u);
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return (a.keys[x] & mask) < (a.keys[y] & mask); });
    for (uint32_t j = 0; j < n; ++j) { a.keys2[j] = a.keys[perm[j]]; a.vals2[j] = a.vals[perm[j]]; }
    launch(flags_thunk);
    std::partial_sum(a.flags, a.flags + n, a.flags);
    launch(rename_thunk);
    ++rounds;
    const uint32_t names = a.flags[n - 1];
    if (zpq::sa_round_is_last(names, n, a.h, n)) break;
    if (rounds >= 40) { fprintf(stderr, "the doubling loop did not end (%u names of %u)\n", names, n); exit(3); }
  }
  launch(invert_thunk);
  launch(bwt_thunk);
  dump(base + ".sa", a.sa, 4ull * n);
  dump(base + ".rank", a.rank, 4ull * n);
  std::vector<uint8_t> stream(a.bwt, a.bwt + n + 1);
  uint32_t idx = a.idx[0];
  for (int b = 0; b < 4; ++b) { stream.push_back((uint8_t)idx); idx >>= 8; }
  dump(base + ".bwt", stream.data(), stream.size());
  printf("block %u n %u bits %u rounds %u\n", k, n, r, rounds);
  fflush(stdout);                                 // (a guard page ends the process: the lines say which block it was)
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "bits" && argc == 3) { printf("bits %u\n", zpq::sa_wide_rank_bits(strtoull(argv[2], nullptr, 10))); return 0; }
  if (mode == "field" && argc == 4) {
    printf("field %u\n", zpq::sa_wide_field_bits((unsigned)strtoul(argv[2], nullptr, 10), (uint32_t)strtoul(argv[3], nullptr, 10)));
    return 0;
  }
  if (mode != "sort" || argc < 5) return usage();
  const unsigned rank_bits = (unsigned)strtoul(argv[2], nullptr, 10);
  const std::string prefix = argv[3];
  for (int at = 4; at < argc; ++at) sort_block((unsigned)(at - 4), slurp(argv[at]), rank_bits, prefix);
  return 0;
}
