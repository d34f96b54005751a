// TEST INFRASTRUCTURE -- LZBuffer's codes from token lists (zpaq_amd/csrc/device/lz77_codes_kernel.h) on the host-side wavefront
// emulator (wave_emu.h): lzc_len_body, a host loop in place of the scan, lzc_sizes_body, the host's placement of the streams, then
// lzc_match_body and lzc_literal_body, for several blocks in one batch as the engine lays them out.
//
//   lz77_codes_emu <kind> <min_match> <rb> <out_prefix> (<input> <tokens>)...
//
// kind 1 / 2: bit-packed / byte-aligned codes; <tokens>: 16 bytes per match (i, off, len, blit).  Prints "error <word>"; with the
// word 0, <out_prefix>.<k> = block k's stream -- otherwise nothing is emitted, as in the engine.
#include "wave_emu.h"

#include <string>
#include <vector>

// the one primitive of the coder's kernels the emulator's header lacks: the fibers of a workgroup share one OS thread and yield
// only at cross-lane operations, so a plain read-modify-write is atomic
static inline unsigned atomicOr(unsigned* p, unsigned v) { const unsigned old = *p; *p = old | v; return old; }

#include "lz77_codes_kernel.h"

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
  const zpq::LzBlock* blocks;
  uint32_t nblocks;
  uint64_t total, nslots;
  const zpq::LzTok* toks;
  const uint32_t* counts;
  uint64_t* pos;
  uint32_t* sizes;
  const uint64_t* out_off;
  uint8_t* out;
};

void len_thunk(void* p) { Args* a = (Args*)p; zpq::lzc_len_body(a->blocks, a->nblocks, a->nslots, a->toks, a->counts, a->pos, a->sizes + a->nblocks); }
void sizes_thunk(void* p) { Args* a = (Args*)p; zpq::lzc_sizes_body(a->blocks, a->nblocks, a->nslots, a->pos, a->sizes); }
void match_thunk(void* p) { Args* a = (Args*)p; zpq::lzc_match_body(a->blocks, a->nblocks, a->nslots, a->toks, a->counts, a->pos, a->out_off, a->out); }
void literal_thunk(void* p) {
  Args* a = (Args*)p;
  zpq::lzc_literal_body(a->in_all, a->blocks, a->nblocks, a->total, a->toks, a->counts, a->pos, a->out_off, a->out);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 7 || ((argc - 5) & 1)) {
    fprintf(stderr, "usage: lz77_codes_emu <kind> <min_match> <rb> <out_prefix> (<input> <tokens>)...\n");
    return 2;
  }
  const uint32_t kind = (uint32_t)atoi(argv[1]), min_match = (uint32_t)atoi(argv[2]), rb = (uint32_t)atoi(argv[3]);
  const std::string prefix = argv[4];
  const unsigned nb = (unsigned)(argc - 5) / 2;
  if ((kind != 1 && kind != 2) || min_match < 1 || rb > 7) { fprintf(stderr, "parameters outside the device coder's range\n"); return 2; }
  std::vector<zpq::LzBlock> blocks(nb);
  std::vector<uint8_t> in_all;
  std::vector<zpq::LzTok> toks;
  std::vector<uint32_t> counts(nb);
  for (unsigned b = 0; b < nb; ++b) {
    const std::vector<uint8_t> in = slurp(argv[5 + 2 * b]), tk = slurp(argv[6 + 2 * b]);
    if (in.size() >= (1u << 24) || tk.size() % 16) { fprintf(stderr, "block %u outside the range\n", b); return 2; }
    zpq::LzBlock& B = blocks[b];
    memset(&B, 0, sizeof B);
    B.off = in_all.size();
    B.n = (uint32_t)in.size();
    B.kind = kind;                                // (also for an empty block: a list over it must be refused)
    B.min_match = min_match;
    B.rb = rb;
    B.tok_off = toks.size();
    B.tok_cap = (uint32_t)(tk.size() / 16);
    counts[b] = B.tok_cap;
    toks.resize(toks.size() + B.tok_cap);
    if (!tk.empty()) memcpy(toks.data() + B.tok_off, tk.data(), tk.size());
    in_all.insert(in_all.end(), in.begin(), in.end());
  }
  const uint64_t total = in_all.size(), nslots = toks.size() + nb;
  in_all.resize(total + 64, 0xA5);                // (nothing may depend on what lies behind the batch)
  toks.resize(toks.size() + 1);
  std::vector<uint64_t> pos(nslots + 2, ~0ull);
  std::vector<uint32_t> sizes(nb + 2, 0);
  sizes[nb + 1] = 0xFFFFFFFFu;
  Args a{in_all.data(), blocks.data(), nb, total, nslots, toks.data(), counts.data(), pos.data(), sizes.data(), nullptr, nullptr};
  const unsigned swgs = (unsigned)((nslots + 1 + 255) / 256), pwgs = (unsigned)((total + 255) / 256);
  for (unsigned wg = 0; wg < swgs; ++wg) emu::run_workgroup(len_thunk, &a, 256, wg);
  if (pos[nslots + 1] != ~0ull || sizes[nb + 1] != 0xFFFFFFFFu) { fprintf(stderr, "the length kernel wrote past its arrays\n"); return 3; }
  uint64_t run = 0;                               // the exclusive scan (rocPRIM on the device)
  for (uint64_t s = 0; s <= nslots; ++s) {
    if (pos[s] == ~0ull) { fprintf(stderr, "length %llu was never written\n", (unsigned long long)s); return 3; }
    const uint64_t l = pos[s];
    pos[s] = run;
    run += l;
  }
  for (unsigned wg = 0; wg < (nb + 255) / 256; ++wg) emu::run_workgroup(sizes_thunk, &a, 256, wg);
  printf("error %u\n", sizes[nb]);
  if (sizes[nb]) return 0;
  std::vector<uint64_t> out_off(nb + 1, 0);       // the host's placement: back to back, every start on a word
  for (unsigned b = 0; b < nb; ++b) out_off[b + 1] = out_off[b] + (((uint64_t)sizes[b] + 3) & ~3ull);
  std::vector<uint8_t> out(out_off[nb] + 64, 0);
  memset(out.data() + out_off[nb], 0x5A, 64);
  a.out_off = out_off.data();
  a.out = out.data();
  for (unsigned wg = 0; wg < (unsigned)((nslots + 255) / 256); ++wg) emu::run_workgroup(match_thunk, &a, 256, wg);
  for (unsigned wg = 0; wg < pwgs; ++wg) emu::run_workgroup(literal_thunk, &a, 256, wg);
  for (unsigned k = 0; k < 64; ++k)
    if (out[out_off[nb] + k] != 0x5A) { fprintf(stderr, "the emitting kernels wrote past the output\n"); return 3; }
  for (unsigned b = 0; b < nb; ++b) {
    for (uint64_t k = out_off[b] + sizes[b]; k < out_off[b + 1]; ++k)
      if (out[k]) { fprintf(stderr, "block %u: a store behind its stream\n", b); return 3; }
    const std::string path = prefix + "." + std::to_string(b);
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { perror(path.c_str()); return 2; }
    fwrite(out.data() + out_off[b], 1, sizes[b], f);
    fclose(f);
    printf("block %u n %u tokens %u bytes %u\n", b, blocks[b].n, counts[b], sizes[b]);
  }
  return 0;
}
