// TEST INFRASTRUCTURE -- the LZ77 parse through LZBuffer's hash table (zpaq_amd/csrc/device/lz77_hash_kernel.h) on the host-side
// wavefront emulator (wave_emu.h): lzh_keys_body, a host sort in place of the radix sort, lzh_index_body, lzh_search_body and
// the walk of lz77_kernel.h, for several blocks in one batch as the engine lays them out.
//
//   lz77_hash_emu <kind> <min_match> <min_match2> <lookahead> <bucket> <checkbits> <ht_bits> <idx_bits|-1> <out_prefix> <input>...
//
// kind 1 / 2: bit-packed / byte-aligned codes; idx_bits -1: the index the engine would build (layout.h lz_hash_plan), else that
// many bits (clamped to what a bucket allows).  <out_prefix>.<k> = block k's token list (16 bytes per match).
#include "wave_emu.h"

#include <algorithm>
#include <string>
#include <vector>

#include "lz77_hash_kernel.h"

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
  uint64_t total, nkeys;
  uint16_t* blk;
  uint64_t *keys, *sorted;
  uint32_t* idx;
  uint4* res;
  zpq::LzTok* toks;
  uint32_t* counts;
};

void keys_thunk(void* p) { Args* a = (Args*)p; zpq::lzh_keys_body(a->in_all, a->blocks, a->nblocks, a->total, a->blk, a->keys); }
void index_thunk(void* p) { Args* a = (Args*)p; zpq::lzh_index_body(a->sorted, a->nkeys, a->blocks, a->idx); }
void search_thunk(void* p) { Args* a = (Args*)p; zpq::lzh_search_body(a->in_all, a->sorted, a->idx, a->blk, a->blocks, a->total, a->res); }
void walk_thunk(void* p) { Args* a = (Args*)p; zpq::lz77_walk_body(a->blocks, a->res, a->toks, a->counts); }

}  // namespace

int main(int argc, char** argv) {
  if (argc < 11) {
    fprintf(stderr, "usage: lz77_hash_emu <kind> <min_match> <min_match2> <lookahead> <bucket> <checkbits> <ht_bits> <idx_bits|-1> <out_prefix> <input>...\n");
    return 2;
  }
  const uint32_t kind = (uint32_t)atoi(argv[1]), min_match = (uint32_t)atoi(argv[2]), min_match2 = (uint32_t)atoi(argv[3]),
                 lookahead = (uint32_t)atoi(argv[4]), bucket = (uint32_t)atoi(argv[5]), checkbits = (uint32_t)atoi(argv[6]),
                 ht_bits = (uint32_t)atoi(argv[7]);
  const int idx_bits = atoi(argv[8]);
  const std::string prefix = argv[9];
  const unsigned nb = (unsigned)(argc - 10);
  if ((kind != 1 && kind != 2) || min_match < 2 || ht_bits < 1 || ht_bits > zpq::kLzhMaxTableBits || bucket >= (1u << ht_bits)) {
    fprintf(stderr, "parameters outside the device parser's range\n");
    return 2;
  }
  std::vector<zpq::LzBlock> blocks(nb);
  std::vector<uint8_t> in_all;
  uint64_t ntok = 0, nkeys = 0, nidx = 0;
  for (unsigned b = 0; b < nb; ++b) {
    const std::vector<uint8_t> in = slurp(argv[10 + b]);
    zpq::LzBlock& B = blocks[b];
    memset(&B, 0, sizeof B);
    B.off = in_all.size();
    B.n = (uint32_t)in.size();
    B.kind = in.empty() ? 0u : kind;
    B.min_match = min_match; B.lookahead = lookahead; B.bucket = bucket; B.checkbits = checkbits;
    B.min_match2 = min_match2; B.ht_bits = ht_bits;
    B.tok_off = ntok;
    B.tok_cap = B.n / min_match + 2u;
    ntok += B.tok_cap;
    const uint64_t idx_at = nidx;
    zpq::lz_hash_plan(B, nkeys, nidx);
    if (idx_bits >= 0) {                          // (a coarser or finer index than the engine's: the answers must not depend on it)
      uint32_t bucket_bits = 0;
      while ((1u << bucket_bits) <= bucket) ++bucket_bits;
      B.idx_bits = std::min((uint32_t)idx_bits, ht_bits - bucket_bits);
      nidx = idx_at + (1ull << B.idx_bits) + 1u;
    }
    in_all.insert(in_all.end(), in.begin(), in.end());
  }
  const uint64_t total = in_all.size();
  in_all.resize(total + 64, 0xA5);             // (the engine's input buffer is padded as well; nothing may depend on what lies there)
  std::vector<uint16_t> blk(total + 1, 0xFFFF);
  std::vector<uint64_t> keys(nkeys + 1, ~0ull), sorted;
  std::vector<uint32_t> idx(nidx + 1, 0xFFFFFFFFu);
  std::vector<uint4> res(total + 1);
  std::vector<zpq::LzTok> toks(ntok + 1);
  std::vector<uint32_t> counts(nb, 0);
  Args a{in_all.data(), blocks.data(), nb, total, nkeys, blk.data(), keys.data(), nullptr, idx.data(), res.data(), toks.data(), counts.data()};
  const unsigned wgs = (unsigned)((total + 255) / 256), kwgs = (unsigned)((nkeys + 255) / 256);
  for (unsigned wg = 0; wg < wgs; ++wg) emu::run_workgroup(keys_thunk, &a, 256, wg);
  if (keys[nkeys] != ~0ull) { fprintf(stderr, "the key kernel wrote past its array\n"); return 3; }
  for (uint64_t k = 0; k < nkeys; ++k)
    if (keys[k] == ~0ull) { fprintf(stderr, "key %llu was never written\n", (unsigned long long)k); return 3; }
  sorted.assign(keys.begin(), keys.begin() + nkeys);
  std::sort(sorted.begin(), sorted.end());
  sorted.push_back(~0ull);
  a.sorted = sorted.data();
  for (unsigned wg = 0; wg < kwgs; ++wg) emu::run_workgroup(index_thunk, &a, 256, wg);
  if (idx[nidx] != 0xFFFFFFFFu) { fprintf(stderr, "the index kernel wrote past its array\n"); return 3; }
  for (unsigned b = 0; b < nb; ++b) {           // every entry of a block with keys is written, and they never decrease
    const zpq::LzBlock& B = blocks[b];
    if (!B.nkeys || !B.n) continue;
    for (uint64_t c = 0; c <= (1ull << B.idx_bits); ++c) {
      const uint32_t v = idx[B.idx_off + c];
      if (v > B.nkeys || (c && v < idx[B.idx_off + c - 1])) { fprintf(stderr, "block %u: index entry %llu = %u\n", b, (unsigned long long)c, v); return 3; }
    }
    if (idx[B.idx_off] != 0 || idx[B.idx_off + (1ull << B.idx_bits)] != B.nkeys) { fprintf(stderr, "block %u: index ends\n", b); return 3; }
  }
  for (unsigned wg = 0; wg < wgs; ++wg) emu::run_workgroup(search_thunk, &a, 256, wg);
  for (unsigned b = 0; b < nb; ++b) emu::run_workgroup(walk_thunk, &a, 64, b);
  for (unsigned b = 0; b < nb; ++b) {
    const std::string path = prefix + "." + std::to_string(b);
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { perror(path.c_str()); return 2; }
    const zpq::LzBlock& B = blocks[b];
    if (counts[b] > B.tok_cap) { fprintf(stderr, "block %u: %u tokens for %u slots\n", b, counts[b], B.tok_cap); return 3; }
    fwrite(toks.data() + B.tok_off, 16, counts[b], f);
    fclose(f);
    printf("block %u n %u keys %u idx_bits %u tokens %u\n", b, B.n, B.nkeys, B.idx_bits, counts[b]);
  }
  return 0;
}
