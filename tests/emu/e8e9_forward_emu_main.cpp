// TEST INFRASTRUCTURE -- the forward E8E9 filter (zpaq_amd/csrc/device/e8e9_forward_kernel.h) on the host-side wavefront emulator
// (wave_emu.h): the blocks back to back at whatever offsets their lengths give, as the sorters' batches lie, the buffer ending
// where an inaccessible page starts, the mark pass, the scan over the tiles' counts (the
// engine runs rocPRIM's there), the list sized from the two totals, the scatter and the walk, for several blocks in one batch.
// Every array has its exact size between inaccessible pages (guard_alloc.h) and starts dirty.
//
//   e8e9_forward_emu run <max_steps> <out_prefix> <block>...        max_steps 0: the engine's cap (kE8MaxSteps)
//
// Prints "block <k> status <s> out_len <n> steps_cap <c>" per block; <out_prefix>.<k> = block k filtered, for those with status 0.
#include "wave_emu.h"

#include <string>
#include <vector>

#include "e8e9_forward_kernel.h"
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
  uint8_t* buf;
  const zpq::E8Block* blocks;
  uint32_t nblocks, ntiles, nseeds, max_steps;
  uint32_t* cnt;
  uint32_t* list;
  uint32_t* status;
};

void mark_thunk(void* p) { Args* a = (Args*)p; zpq::e8f_mark_body(a->buf, a->blocks, a->nblocks, a->ntiles, a->cnt, a->status); }
void scatter_thunk(void* p) { Args* a = (Args*)p; zpq::e8f_scatter_body(a->buf, a->blocks, a->nblocks, a->ntiles, a->cnt, a->list); }
void walk_thunk(void* p) {
  Args* a = (Args*)p;
  zpq::e8f_walk_body(a->buf, a->blocks, a->nblocks, a->ntiles, a->cnt, a->list, a->nseeds, a->max_steps, a->status);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 5 || strcmp(argv[1], "run")) {
    fprintf(stderr, "usage: e8e9_forward_emu run <max_steps> <out_prefix> <block>...\n");
    return 2;
  }
  const uint32_t max_steps = atoi(argv[2]) > 0 ? (uint32_t)atoi(argv[2]) : zpq::kE8MaxSteps;
  const std::string prefix = argv[3];
  const unsigned nb = (unsigned)(argc - 4);
  std::vector<std::vector<uint8_t>> in(nb);
  std::vector<zpq::E8Block> bl(nb);
  uint64_t room = 0, tiles = 0;
  for (unsigned b = 0; b < nb; ++b) {
    in[b] = slurp(argv[4 + b]);
    bl[b].off = room;
    bl[b].n = (uint32_t)in[b].size();
    bl[b].tile_off = (uint32_t)tiles;
    room += in[b].size();
    tiles += zpq::e8_tiles(bl[b].n);
  }
  Args a;
  a.buf = emu::guard_alloc(room, 1, 0xA5);
  for (unsigned b = 0; b < nb; ++b) if (!in[b].empty()) memcpy(a.buf + bl[b].off, in[b].data(), in[b].size());
  zpq::E8Block* blocks = (zpq::E8Block*)emu::guard_alloc(sizeof(zpq::E8Block) * nb, 8, 0);
  memcpy(blocks, bl.data(), sizeof(zpq::E8Block) * nb);
  a.blocks = blocks;
  a.nblocks = nb;
  a.ntiles = (uint32_t)tiles;
  a.max_steps = max_steps;
  a.cnt = (uint32_t*)emu::guard_alloc(4 * (2 * tiles + 1), 4, 0xEE);
  a.status = (uint32_t*)emu::guard_alloc(4 * nb, 4, 0xEE);
  a.list = nullptr;
  a.nseeds = 0;
  for (unsigned g = 0; g < tiles; ++g) emu::run_workgroup(mark_thunk, &a, 256, g);
  uint32_t run = 0;                                             // the exclusive scan, in place
  for (uint64_t k = 0; k < 2 * tiles + 1; ++k) { const uint32_t c = a.cnt[k]; a.cnt[k] = run; run += c; }
  a.nseeds = a.cnt[tiles];
  const uint32_t nlist = a.cnt[2 * tiles];
  if (a.nseeds) {
    a.list = (uint32_t*)emu::guard_alloc(4 * (size_t)nlist, 4, 0xEE);
    for (unsigned g = 0; g < tiles; ++g) emu::run_workgroup(scatter_thunk, &a, 256, g);
    for (unsigned g = 0; g < (a.nseeds + 255u) / 256u; ++g) emu::run_workgroup(walk_thunk, &a, 256, g);
  }
  for (unsigned b = 0; b < nb; ++b) {
    const bool ok = a.status[b] == 0u;
    printf("block %u status %u out_len %u steps_cap %u\n", b, a.status[b], ok ? bl[b].n : 0u, max_steps);
    if (!ok) continue;
    const std::string path = prefix + "." + std::to_string(b);
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { perror(path.c_str()); return 2; }
    fwrite(a.buf + bl[b].off, 1, bl[b].n, f);
    fclose(f);
  }
  return 0;
}
