#include "launch_policy.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "../host/codegen.hpp"

namespace zpq {

LaunchKnobs launch_knobs() {
  LaunchKnobs k;
  if (const char* v = getenv("ZPAQ_AMD_PIPE_PERSIST")) k.persist = !strcmp(v, "0") ? LaunchKnobs::kPersistOff : LaunchKnobs::kPersistForced;
  if (const char* v = getenv("ZPAQ_AMD_PIPE_MODE"))
    k.mode = !strcmp(v, "latency") ? LaunchKnobs::kModeLatency : (!strcmp(v, "throughput") ? LaunchKnobs::kModeThroughput : LaunchKnobs::kModeOther);
  if (const char* v = getenv("ZPAQ_AMD_PIPE_WIDE")) k.wide_off = v[0] == '0';
  k.profile = getenv("ZPAQ_AMD_PIPE_PROFILE") != nullptr;
  if (const char* v = getenv("ZPAQ_AMD_PIPE_TRACE")) { k.trace = true; k.trace_path = v; }
  if (const char* v = getenv("ZPAQ_AMD_PERSIST_TIMEOUT_MS")) k.timeout_ms = (uint32_t)std::max(1, atoi(v));
  if (const char* v = getenv("ZPAQ_AMD_PERSIST_ARRIVE_MS")) k.arrive_ms = (uint32_t)std::max(1, atoi(v));
  if (const char* v = getenv("ZPAQ_AMD_PERSIST_SPREAD")) k.spread = atoi(v) == 8 ? 1 : 0;
  return k;
}

// The pipelined encoder has two shapes per chain (host/codegen.hpp PipeOptions): a chain with few blocks in the batch is
// latency bound -- a step costs one wavefront's serial chain however empty the machine is -- and runs the units with a
// lane per bit position; a chain that fills the machine is bound by HBM transactions and runs the lane-per-block units,
// which issue fewer requests.  Measured crossover on the MI355X, -m5 / 1 MiB blocks, 8 hardware queues: latency mode is
// 1.40 x faster at 64 blocks, 1.07 x at 512, 0.95 x at 768, 0.86 x at 1024 (profiles/r03/call6_summary.txt).
static const uint32_t kLongStepBytes = 128u << 10;       // latency shape: blocks this long may take 2048-byte steps (codegen.hpp)
// ... when what the units of one step pass each other stays small: a step's streams (blocks x 2048 bytes x the chain's
// ctx / bh / p bytes per input byte) are written and read once within a few steps, and up to ~100 MB of them live in the
// 256 MB Infinity Cache instead of HBM.  Measured (profiles/r03/call10_summary.txt): -m3's n = 2 chain on 256 blocks
// (29 MB per step) 483 -> 440 ms; -m5 (588 B per byte) +4 % at 64 blocks (77 MB), +6 % at 512 (616 MB), -20 % at 640.
static const uint64_t kLongStepStreamBytes = 96ull << 20;

// a chain's layout in variant v when the persistent launch can pack it, else nullptr
static const PipeLayout* packed_layout(const zpq_plan* plan, int v) {
  const PipeLayout* L = plan_pipe_layout(*plan, v);
  return L && L->persist_ok ? L : nullptr;
}
static uint64_t groups_of(uint32_t blocks, const PipeLayout* L) { return (blocks + (uint32_t)L->G - 1) / (uint32_t)L->G; }

// bytes the units of a chain pass each other per input byte (ctx 4, bh 8, p 16 per stream); 0: no pipelined encoder
static uint32_t pipe_stream_bytes_per_byte(const zpq_plan* plan) {
  const PipeLayout* L = plan_pipe_layout(*plan, 1);
  return L ? (uint32_t)(L->nctx * 4 + L->nrow * 8 + L->n * 16) : 0u;
}

// the variant of one chain that has the device to itself
static int variant_alone(const DeviceShape& dev, const LaunchKnobs& knobs, bool persist_expected, const ChainLoad& c) {
  bool latency = c.blocks <= kLatencyModeBlocks;
  bool persist_off = knobs.persist == LaunchKnobs::kPersistOff || !persist_expected;
  // With the persistent launch the shapes differ in how many workgroups a group of blocks needs (-m5: 14 against 8): the
  // latency shape is the faster one exactly while ALL its workgroups are resident together (measured, profiles/r05
  // call13: 512 blocks 268 MB/s against 187; beyond that -- 640 blocks: 280 workgroups -- it would need a second round,
  // which costs a whole block's serial time, and the throughput shape in one round wins: 768 blocks 264 MB/s, 1024: 350)
  const PipeLayout* L1 = persist_off ? nullptr : packed_layout(c.plan, 1);
  if (L1) latency = groups_of(c.blocks, L1) * (uint64_t)L1->ps_wpg <= (uint64_t)dev.cus;
  else persist_off = true;           // (a chain that cannot be packed: the step kernels, by round 4's rule)
  if (knobs.mode == LaunchKnobs::kModeLatency) latency = true;
  if (knobs.mode == LaunchKnobs::kModeThroughput) latency = false;
  if (!latency) return 0;
  // (long steps exist to spread the per-step launch cost; the persistent launch has none and takes the 512-byte shape)
  const uint32_t stream_bytes_per_byte = pipe_stream_bytes_per_byte(c.plan);
  if (persist_off && c.longest >= kLongStepBytes && stream_bytes_per_byte &&
      (uint64_t)c.blocks * 2048u * stream_bytes_per_byte <= kLongStepStreamBytes)
    return 2;
  // Variant 3: the latency shape with a wavefront per SIMD (twice the workgroups per group) while THOSE all fit the device
  // (round 6, call 29: -m5 on 64 / 128 / 256 blocks +17 / +20 / +26 %); a small chain's variant 1 is that shape already.
  if (!persist_off && !knobs.wide_off && knobs.mode == LaunchKnobs::kModeAuto) {
    const PipeLayout* L3 = packed_layout(c.plan, 3);
    if (L3 && L3->ps_waves < L1->ps_waves && groups_of(c.blocks, L3) * (uint64_t)L3->ps_wpg <= (uint64_t)dev.cus) return 3;
  }
  return 1;
}

std::vector<int> encoder_variants(const DeviceShape& dev, const LaunchKnobs& knobs, bool persist_expected, const std::vector<ChainLoad>& chains) {
  std::vector<int> mode(chains.size());
  for (size_t i = 0; i < chains.size(); ++i) mode[i] = variant_alone(dev, knobs, persist_expected, chains[i]);
  if (chains.size() < 2) return mode;
  // (several chains in one batch: variant 3's workgroups are not part of the arithmetic below -- variant 1 there)
  for (int& m : mode) if (m == 3) m = 1;
  // several chains in one batch share the device's workgroup slots: the persistent launches run side by side only when they
  // are resident TOGETHER, so chains go from the latency shape to the throughput shape (fewer workgroups per group), the one
  // that frees the most first, until the batch fits
  if (knobs.persist == LaunchKnobs::kPersistOff || !persist_expected || knobs.mode != LaunchKnobs::kModeAuto) return mode;
  struct Need { uint64_t lat, thr; };      // what an XCD has to hold of the chain in either shape
  std::vector<Need> need;
  for (const ChainLoad& c : chains) {
    const PipeLayout *L0 = packed_layout(c.plan, 0), *L1 = packed_layout(c.plan, 1);
    if (!L0 || !L1) return mode;
    const uint64_t groups = groups_of(c.blocks, L0);
    need.push_back(Need{persist_xcd_share(dev, groups, (uint64_t)L1->ps_wpg), persist_xcd_share(dev, groups, (uint64_t)L0->ps_wpg)});
  }
  for (;;) {
    uint64_t total = 0;
    for (size_t i = 0; i < need.size(); ++i) total += mode[i] == 0 ? need[i].thr : need[i].lat;
    if (total <= (uint64_t)dev.cus / (uint64_t)dev.xcds) break;             // (persist_runs_fit's rule: every XCD's share of every run fits)
    size_t best = need.size();
    for (size_t i = 0; i < need.size(); ++i)
      if (mode[i] != 0 && need[i].lat > need[i].thr && (best == need.size() || need[i].lat - need[i].thr > need[best].lat - need[best].thr)) best = i;
    if (best == need.size()) break;
    mode[best] = 0;
  }
  return mode;
}

bool persist_wanted(const LaunchKnobs& knobs, bool eligible) {
  return eligible && knobs.persist != LaunchKnobs::kPersistOff && !knobs.profile && !knobs.trace;
}

PersistRounds persist_rounds(uint32_t capacity, uint32_t wpg, uint32_t groups) {
  const uint32_t most = std::max<uint32_t>(1u, capacity / wpg), rounds = (groups + most - 1) / most;
  return PersistRounds{most, rounds, (groups + rounds - 1) / rounds};
}

bool persist_rounds_worth(const LaunchKnobs& knobs, const PersistRounds& r, uint32_t groups) {
  return r.rounds == 1 || (double)groups / ((double)r.rounds * r.most) >= 0.85 || knobs.persist == LaunchKnobs::kPersistForced;
}

uint32_t persist_xcd_share(const DeviceShape& dev, uint64_t groups, uint64_t wpg) {
  const uint64_t x = (uint64_t)dev.xcds;
  if (groups >= x) return (uint32_t)((groups / x) * wpg + ((groups % x) * wpg + x - 1) / x);
  return (uint32_t)((groups * wpg + x - 1) / x);
}

// The dispatcher does not look for room elsewhere.  (Measured with the archiver's batch of 14 + 2 groups, calls 24-27: sized
// against the device as a whole -- 238 of 256 compute units -- the short run found 2 free compute units per XCD on six XCDs
// where it needed 3-4, sat half resident until the long one ended, and the batch took the sum of both: 3.2 s instead of 1.7.)
bool persist_runs_fit(const DeviceShape& dev, const std::vector<PersistRun>& runs) {
  uint32_t share = 0, room = 0xFFFFFFFFu;
  for (const PersistRun& r : runs) {
    share += persist_xcd_share(dev, r.groups, r.wpg);
    room = std::min(room, r.capacity / (uint32_t)dev.xcds);
  }
  return share <= room;
}

uint32_t persist_spread(const DeviceShape& dev, const LaunchKnobs& knobs, uint32_t groups) {
  const bool on = knobs.spread >= 0 ? knobs.spread != 0 : groups >= (uint32_t)dev.xcds;
  return on ? (uint32_t)dev.xcds : 1u;
}

uint32_t persist_ticks(uint32_t ms) { return (uint32_t)std::min<uint64_t>((uint64_t)ms * 100000ull, 0xFFFFFFF0ull); }

}  // namespace zpq
