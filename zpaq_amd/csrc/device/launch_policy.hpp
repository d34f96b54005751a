// Launch policy of the pipelined encoder: which variant (host/codegen.hpp pipe_options: 0 throughput, 1 latency, 2 long steps,
// 3 wide) codes each chain of a batch, and whether the batch goes as one persistent launch per chain or as the six step
// kernels.  Host only, no HIP call: every rule is a function of the device's shape, the knobs of the environment and numbers
// the engine hands in (device/engine.cpp keeps the launches, the streams and the abort handling).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

struct zpq_plan;

namespace zpq {

struct DeviceShape { int cus = 256; int xcds = 8; };      // compute units, and the compute dies (XCDs) they sit on

// The engine-side knobs.  Read once per engine call (at the entry of the call that builds the launch groups) and passed
// down; not kept between calls: a test may change the environment from one call to the next.
struct LaunchKnobs {
  enum Persist { kPersistAuto, kPersistOff, kPersistForced };
  enum Mode { kModeAuto, kModeLatency, kModeThroughput, kModeOther };
  Persist persist = kPersistAuto;   // ZPAQ_AMD_PIPE_PERSIST: unset / "0" / any other value (which also overrides the round-fill rule)
  Mode mode = kModeAuto;            // ZPAQ_AMD_PIPE_MODE=latency|throughput (A/B, tests); set to anything, it also disables variant 3
                                    // and the demotion of chains that share the device
  bool wide_off = false;            // ZPAQ_AMD_PIPE_WIDE=0: no variant 3
  bool profile = false;             // ZPAQ_AMD_PIPE_PROFILE present: every unit type of every step alone, timed
  bool trace = false;               // ZPAQ_AMD_PIPE_TRACE present: one record per workgroup and launch ...
  std::string trace_path;           // ... written to this file
  uint32_t timeout_ms = 3000;       // ZPAQ_AMD_PERSIST_TIMEOUT_MS: the persistent launch's watchdog
  // ZPAQ_AMD_PERSIST_ARRIVE_MS: how long the workgroups of a launch may wait for each other to become resident (pipe_persist.h
  // pipe_arrived) before the launch is given up untouched: 20 ms without a new arrival (a full grid arrives within microseconds of
  // its first workgroup; measured with 200 of 256 compute units held by another process, profiles/r06: the engine knows ~2 x this
  // after the launch -- the workgroups that were left in the queue still have to be dispatched, see the flag and leave)
  uint32_t arrive_ms = 20;
  int spread = -1;                  // ZPAQ_AMD_PERSIST_SPREAD (experiments): -1 unset, 1 = "8" (a group's workgroups share an XCD), 0 = any other value
};
LaunchKnobs launch_knobs();

// ---- the variant of every chain of a batch ----
struct ChainLoad {
  const zpq_plan* plan = nullptr;
  uint32_t blocks = 0;     // blocks of the batch that carry this chain
  uint32_t longest = 0;    // bytes of the longest of them
};
// persist_expected: the call will take the persistent launch if the chain can (it waits for its results: zpq_*_device with timed = 0
// returns with the work in flight and runs the step kernels) -- the shape is chosen for the launch form that will really run.
// One variant per chain, in the order given (which also breaks ties when chains are demoted).
std::vector<int> encoder_variants(const DeviceShape& dev, const LaunchKnobs& knobs, bool persist_expected, const std::vector<ChainLoad>& chains);
static const uint32_t kLatencyModeBlocks = 640;      // a residency wave with fewer blocks may get one of the latency shapes

// ---- the launch form ----
// eligible: every group of the batch is a pipelined one whose chain has a persistent kernel, and the call waits for its results
bool persist_wanted(const LaunchKnobs& knobs, bool eligible);
// A run of `groups` groups x `wpg` workgroups on a device that holds `capacity` (>= wpg) workgroups of its kernel at once: all
// workgroups of a launch must be resident together, so a run with more groups goes in rounds
struct PersistRounds { uint32_t most, rounds, per_round; };      // groups resident together; launches; groups in each (equal sizes)
PersistRounds persist_rounds(uint32_t capacity, uint32_t wpg, uint32_t groups);
// a single run: one round, or rounds that are nearly full (a round costs a block's serial time whatever it holds), or forced
bool persist_rounds_worth(const LaunchKnobs& knobs, const PersistRounds& r, uint32_t groups);
// Workgroups of a persistent launch of `groups` groups x `wpg` workgroups that one XCD gets (the dispatcher deals a launch's
// workgroups round-robin over the XCDs; pipe_persist.h maps whole sets of one group per XCD, the rest in launch order)
uint32_t persist_xcd_share(const DeviceShape& dev, uint64_t groups, uint64_t wpg);
// several runs go side by side or not at all: every XCD's share of every run has to fit
struct PersistRun { uint32_t groups, wpg, capacity; };
bool persist_runs_fit(const DeviceShape& dev, const std::vector<PersistRun>& runs);
// PipeArgs::spread of a launch of `groups` groups: a group's workgroups that far apart in the grid, so that they share an XCD
uint32_t persist_spread(const DeviceShape& dev, const LaunchKnobs& knobs, uint32_t groups);
uint32_t persist_ticks(uint32_t ms);      // of the 100 MHz clock the kernels read (timeout_ms, arrive_ms)

}  // namespace zpq
