// What the engine's translation units share: engine.cpp (the coder engine: device set-up, kernel choice, the launches, the
// submission queue), engine_prep.cpp and engine_post.cpp (the batch stages of the compression and the decompression side).
// Private to device/engine*.cpp: engine.hpp is the public header and does not include this one.
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "engine.hpp"
#include "launch_policy.hpp"

namespace zpq {

#define HIP_CHECK(expr)                                                                       \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      int code_ = (e_ == hipErrorOutOfMemory) ? ZPQ_E_NOMEM : ZPQ_E_DEVICE;                   \
      fail(code_, std::string(#expr) + ": " + hipGetErrorString(e_));                         \
    }                                                                                         \
  } while (0)

namespace engine_detail {

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  void ensure(size_t n) {
    if (n <= cap) return;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    size_t want = align_up(n, (size_t)1 << 21);
    HIP_CHECK(hipMalloc(&p, want));
    cap = want;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// Page-locked host memory (ZPAQ_AMD_PINNED_STAGE): the staging buffer of host-buffer batches, DMA-able at link speed
struct HostPinned {
  void* p = nullptr;
  size_t cap = 0;
  bool ensure(size_t n) {                 // false: not available (the caller stages through pageable memory)
    if (n <= cap) return true;
    if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
    size_t want = align_up(n, (size_t)1 << 21);
    if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return false; }
    cap = want;
    return true;
  }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

// hipEvent_t that cannot leak when a HIP_CHECK throws between create and destroy
struct Event {
  hipEvent_t ev = nullptr;
  explicit Event(bool timing = false) {
    HIP_CHECK(hipEventCreateWithFlags(&ev, timing ? hipEventDefault : hipEventDisableTiming));
  }
  ~Event() { if (ev) (void)hipEventDestroy(ev); }
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  operator hipEvent_t() const { return ev; }
};

struct Engine {
  std::mutex mu;
  bool ready = false;
  int device = -1;                     // HIP device this engine drives
  int slot = 0;                        // its index in g_engines = the slot of every plan's per-engine state (zpq_plan::dev[])
  hipStream_t stream = nullptr;
  DeviceTables* d_tables = nullptr;
  uint64_t budget = 0;
  unsigned sharers = 1;          // engines configured on this engine's physical device (ZPAQ_AMD_DEVICES may name one twice)
  int kernel_choice = 0;
  DevBuf arena, io_in, io_out, jobs, results;
  DevBuf segs;                         // segment tables of multi-segment blocks
  DevBuf sha_jobs, sha_out;            // SHA-1 of the staged inputs (sha1_blocks_kernel)
  DevBuf pipe;                         // stream buffers of the pipelined encoder (device/pipe_kernel.h)
  DevBuf pipe_ctl;                     // the persistent launch's progress counters, chunk counts and abort words (device/pipe_persist.h)
  HostPinned pin_in;                   // page-locked staging of host inputs, kept between calls (ZPAQ_AMD_PINNED_STAGE=0: pageable)
  HostPinned pin_out;                  // ... and of the outputs of a large batch
  hipStream_t pstream[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // one per pipe kernel
  std::vector<hipStream_t> side;       // extra streams: independent launch groups run concurrently
  Timing last{};
  int last_kind = 0;
  bool last_persist = false;           // the last batch's pipelined groups ran as persistent launches
  double last_persist_abort_ms = 0.0;  // ... or: how long it took until a persistent launch of the last batch was given up (0: none was)
  int jit_left = 0;                    // hipRTC compilations still allowed in the current call
  std::atomic<int> cus{256};           // compute units of the device (atomic: the submission queue reads the primary engine's without its lock)
  int xcds = 8;                        // ... and its compute dies
  DeviceShape shape() const { return DeviceShape{cus.load(), xcds}; }
  hipEvent_t busy = nullptr;           // recorded after the last launch of a call that returned with work in flight
};

// (defined in engine.cpp)
Engine& eng(int slot = -1);                       // the engine of a slot; -1: the primary one
void require_ready(Engine& e, int slot = -1);     // lazy default init
void bind_device(Engine& e);                      // binds the calling thread: HIP's current device and the plan slot the loaders address
void wait_in_flight(Engine& e);                   // blocks until a call that returned with work in flight has drained

// A call's hold on an engine, from where it is constructed to the end of its scope: the engine locked, initialised, bound to the
// calling thread and drained.  Every entry point that touches the engine's buffers takes it through this and through nothing
// else -- a stage that left out wait_in_flight would race a batch still on the stream, silently.
struct EngineCall {
  Engine& e;
  std::lock_guard<std::mutex> lock;
  explicit EngineCall(int slot = -1) : e(eng(slot)), lock(e.mu) {
    require_ready(e, slot);
    bind_device(e);
    wait_in_flight(e);
  }
};

// ---- what the batch stages write alike (engine_prep.cpp, engine_post.cpp) ----

// Carves a device buffer into arrays: take() returns where the next one starts -- the running end rounded up to `align` -- and
// moves the end behind it.  `at` is what has been used so far (what a budget check adds up).
struct Carve {
  uint64_t at = 0;
  uint64_t take(uint64_t bytes, uint64_t align = 256) {
    const uint64_t o = align_up(at, align);
    at = o + bytes;
    return o;
  }
};

// A launch that failed is no error of the call: the stage declines with `what` + HIP's words in `note`, and HIP's sticky error
// is cleared so that the engine stays usable.  true: it failed.
inline bool launch_failed(hipError_t rc, const char* what, std::string& note) {
  if (rc == hipSuccess) return false;
  (void)hipGetLastError();
  note = std::string(what) + hipGetErrorString(rc);
  return true;
}

// One upload of a batch's host inputs: item i is copied to off[i] of a staging buffer, zeros behind it up to the next multiple
// of `pad` (0: none), and the first `bytes` of the buffer go to d_dst on e.stream.  pinned: through the engine's page-locked
// buffer if it is to be had, else (and otherwise) through pageable memory -- which the returned pointer owns: the caller keeps
// it until it has synchronised the stream.
struct HostItem { const uint8_t* p; uint64_t len, off; };
inline std::unique_ptr<uint8_t[]> upload_staged(Engine& e, void* d_dst, const std::vector<HostItem>& items, uint64_t bytes, uint32_t pad, bool pinned) {
  std::unique_ptr<uint8_t[]> pageable;
  if (!bytes) return pageable;
  uint8_t* stage = pinned && e.pin_in.ensure(bytes + 64) ? (uint8_t*)e.pin_in.p : (pageable.reset(new uint8_t[bytes + 64]), pageable.get());
  for (const HostItem& it : items) {
    if (it.len) memcpy(stage + it.off, it.p, it.len);
    if (pad) memset(stage + it.off + it.len, 0, (size_t)(align_up(it.len, pad) - it.len));
  }
  HIP_CHECK(hipMemcpyAsync(d_dst, stage, bytes, hipMemcpyHostToDevice, e.stream));
  return pageable;
}

}  // namespace engine_detail
using namespace engine_detail;

}  // namespace zpq
