// TEST INFRASTRUCTURE -- the batched suffix sort (zpaq_amd/csrc/device/sa_kernel.h, the loop of device/sa_kernels.hip) on the
// host-side wavefront emulator (sa_emu.h: the bodies as the loop runs them, guarded arrays of the exact size, std::stable_sort on
// the masked key and std::partial_sum in place of the library calls).
//
//   sa_emu sort <out_prefix> <input>... [-- <input>...]...
//       every run of inputs up to a "--" is one batch, sorted as the engine lays it out.  Batch t, block k:
//       <out_prefix>.<t>.<k>.sa = the suffix array, <out_prefix>.<t>.<k>.rank = the ranks the loop ends with (little-endian
//       uint32 each); one line "batch <t> blocks <n> rounds <r>" per batch.
//   sa_emu bits <nblocks>                          the key bits the sort is asked for          -> "bits <n>"
//   sa_emu stop <names> <total> <h> <max_len>      the stop rule after the round of step h     -> "stop <0|1>"
#include "sa_emu.h"

#include <string>

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

void dump(const std::string& path, const uint32_t* p, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) { perror(path.c_str()); exit(2); }
  if (n) fwrite(p, 4, n, f);
  fclose(f);
}

int usage() {
  fprintf(stderr, "usage: sa_emu sort <out_prefix> <input>... [-- <input>...]... | bits <nblocks> | stop <names> <total> <h> <max_len>\n");
  return 2;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "bits" && argc == 3) { printf("bits %u\n", zpq::sa_key_bits((uint32_t)strtoul(argv[2], nullptr, 10))); return 0; }
  if (mode == "stop" && argc == 6) {
    printf("stop %d\n", (int)zpq::sa_round_is_last(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10), (uint32_t)strtoul(argv[4], nullptr, 10),
                                                   (uint32_t)strtoul(argv[5], nullptr, 10)));
    return 0;
  }
  if (mode != "sort" || argc < 4) return usage();
  const std::string prefix = argv[2];
  unsigned t = 0;
  for (int at = 3; at < argc; ++t) {
    std::vector<std::vector<uint8_t>> inputs;
    for (; at < argc && strcmp(argv[at], "--") != 0; ++at) inputs.push_back(slurp(argv[at]));
    ++at;
    const sa_emu::Batch B = sa_emu::build(inputs);
    for (uint32_t k = 0; k < B.nblocks; ++k) {
      const std::string base = prefix + "." + std::to_string(t) + "." + std::to_string(k);
      const size_t n = (size_t)(B.off[k + 1] - B.off[k]);
      dump(base + ".sa", n ? B.sa + B.off[k] : nullptr, n);
      dump(base + ".rank", n ? B.rank + B.off[k] : nullptr, n);
    }
    printf("batch %u blocks %u rounds %u\n", t, B.nblocks, B.rounds);
    fflush(stdout);                               // (a guard page ends the process: the lines say which batch it was)
  }
  return 0;
}
