// TEST INFRASTRUCTURE -- the LZ77 parse of one block in pieces (zpaq_amd/csrc/device/lz77_wide_kernel.h) on the host-side
// wavefront emulator (wave_emu.h): search, piece walk, stitch and gather in the order launch_lz77_wide runs them.
//
//   lz77_wide_emu <kind> <min_match> <lookahead> <bucket> <checkbits> <piece>[,<piece>...] <out_prefix> <input> [<input> ...]
//
// Every input is one block, parsed alone: searched once, then walked, stitched and gathered once per piece size.  The suffix
// array comes from the library's host sorter (zpq_suffix_array_host), the rank array is its inverse + 1: what the wide sorter
// ends with (tests/test_emu_sa_wide.py holds it to that).  piece: positions per piece, 0 = one piece that holds the block.
// Every array has its exact size, ends at an inaccessible page (guard_alloc.h) and is dirty (0xA5) at the start.
// <out_prefix>.<k>.<j> = block k's final token list at the j-th piece size (16 bytes per match); one line
// "block <k> n <n> piece <j> tokens <t> pieces <p> whole <a> rejoined <b> own <c>" each.
#include "wave_emu.h"

#include <string>
#include <vector>

#include "guard_alloc.h"
#include "lz77_wide_kernel.h"
#include "zpaq_amd.h"

namespace {

template <class T>
T* guarded(size_t n) { return (T*)emu::guard_alloc(n * sizeof(T), alignof(T), 0xA5); }

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
  zpq::LzWideParams W;
  const uint8_t* in;
  const uint32_t *sa, *rank;
  const zpq::LzBlock* blocks;
  uint4* res;
  zpq::LzTok* prov;
  zpq::LzWidePiece* pieces;
  zpq::LzTok* toks;
  uint32_t tok_cap;
  zpq::LzWideAdopt* adopt;
  zpq::LzWideResult* out;
};

void search_thunk(void* p) { Args* a = (Args*)p; zpq::lz77_wide_search_body(a->in, a->sa, a->rank, a->blocks, a->res); }
void walk_thunk(void* p) { Args* a = (Args*)p; zpq::lz77_wide_walk_body(a->W, a->res, a->prov, a->pieces); }
void stitch_thunk(void* p) { Args* a = (Args*)p; zpq::lz77_wide_stitch_body(a->W, a->res, a->prov, a->pieces, a->toks, a->tok_cap, a->adopt, a->out); }
void gather_thunk(void* p) { Args* a = (Args*)p; zpq::lz77_wide_gather_body(a->W, a->prov, a->adopt, a->toks, a->tok_cap); }

}  // namespace

int main(int argc, char** argv) {
  if (argc < 9) { fprintf(stderr, "usage: lz77_wide_emu <kind> <min_match> <lookahead> <bucket> <checkbits> <piece>[,<piece>...] <out_prefix> <input>...\n"); return 2; }
  const uint32_t kind = (uint32_t)atoi(argv[1]), min_match = (uint32_t)atoi(argv[2]), lookahead = (uint32_t)atoi(argv[3]),
                 bucket = (uint32_t)atoi(argv[4]), checkbits = (uint32_t)atoi(argv[5]);
  std::vector<uint64_t> piece_args;
  for (const char* q = argv[6]; *q;) {
    char* end = nullptr;
    piece_args.push_back(strtoull(q, &end, 10));
    if (end == q) { fprintf(stderr, "piece sizes: a list of numbers\n"); return 2; }
    q = *end == ',' ? end + 1 : end;
  }
  const std::string prefix = argv[7];
  if ((kind != 1 && kind != 2) || min_match < 1 || lookahead > 255 || checkbits < 1 || checkbits > 31) { fprintf(stderr, "parameters outside the parser's range\n"); return 2; }
  for (int at = 8; at < argc; ++at) {
    const unsigned b = (unsigned)(at - 8);
    const std::vector<uint8_t> input = slurp(argv[at]);
    const uint32_t n = (uint32_t)input.size();
    std::vector<uint32_t> hsa(n + 1);
    if (n && zpq_suffix_array_host(input.data(), n, hsa.data()) != 0) { fprintf(stderr, "suffix array: %s\n", zpq_last_error()); return 2; }
    uint8_t* in = guarded<uint8_t>(n);
    uint32_t* sa = guarded<uint32_t>(n);
    uint32_t* rank = guarded<uint32_t>(n);
    if (n) memcpy(in, input.data(), n);
    if (n) memcpy(sa, hsa.data(), 4ull * n);
    for (uint32_t j = 0; j < n; ++j) rank[sa[j]] = j + 1;
    zpq::LzBlock* B = guarded<zpq::LzBlock>(1);
    memset(B, 0, sizeof *B);
    B->n = n; B->kind = kind; B->min_match = min_match; B->lookahead = lookahead; B->bucket = bucket; B->checkbits = checkbits;
    B->tok_cap = n / min_match + 2u;
    Args a;
    a.in = in; a.sa = sa; a.rank = rank; a.blocks = B;
    a.res = guarded<uint4>(n);
    a.tok_cap = B->tok_cap;
    const unsigned wgs = (unsigned)(((uint64_t)n + 255) / 256);
    for (unsigned wg = 0; wg < wgs; ++wg) emu::run_workgroup(search_thunk, &a, 256, wg);
    for (size_t j = 0; j < piece_args.size(); ++j) {
      const std::string path = prefix + "." + std::to_string(b) + "." + std::to_string(j);
      FILE* f = fopen(path.c_str(), "wb");
      if (!f) { perror(path.c_str()); return 2; }
      zpq::LzWideResult r;
      memset(&r, 0, sizeof r);
      if (n) {                                      // (an empty block never reaches the launcher)
        a.W.n = n;
        a.W.piece = zpq::lz_wide_piece_clamp(piece_args[j] ? piece_args[j] : n);
        a.W.npieces = (uint32_t)(((uint64_t)n + a.W.piece - 1) / a.W.piece);
        a.W.slot_cap = zpq::lz_wide_slot_cap(a.W.piece, min_match);
        a.prov = guarded<zpq::LzTok>((size_t)a.W.npieces * a.W.slot_cap);
        a.pieces = guarded<zpq::LzWidePiece>(a.W.npieces);
        a.toks = guarded<zpq::LzTok>(B->tok_cap);
        a.adopt = guarded<zpq::LzWideAdopt>(a.W.npieces);
        a.out = guarded<zpq::LzWideResult>(1);
        for (unsigned k = 0; k < a.W.npieces; ++k) emu::run_workgroup(walk_thunk, &a, 64, k);
        emu::run_workgroup(stitch_thunk, &a, 64, 0);
        for (unsigned k = 0; k < a.W.npieces; ++k) emu::run_workgroup(gather_thunk, &a, 256, k);
        r = *a.out;
        if (r.overflow || r.count > B->tok_cap) { fprintf(stderr, "block %u: %u tokens for %u slots (piece overflow %u)\n", b, r.count, B->tok_cap, r.overflow); return 3; }
        fwrite(a.toks, 16, r.count, f);
      }
      fclose(f);
      printf("block %u n %u piece %u tokens %u pieces %u whole %u rejoined %u own %u\n", b, n, (unsigned)j, r.count, r.pieces, r.how[0], r.how[1], r.how[2]);
      fflush(stdout);                               // (a guard page ends the process: the lines say which block it was)
    }
  }
  return 0;
}
