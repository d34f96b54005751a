// C ABI (include/zpaq_amd.h): converts internal Failure exceptions into status
// codes and implements the batched block-level drop-ins on top of the engine.
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>

#include "device/engine.hpp"
#include "device/launch_policy.hpp"
#include "device/plan.hpp"
#include "device/spec_loader.hpp"
#include "host/codegen.hpp"
#include "host/common.hpp"
#include "host/blocks.hpp"
#include "host/container.hpp"

namespace zpq { std::vector<U8> builtin_model(int level); }      // libzpaq_compat.cpp: the stored headers of min / mid / max.cfg

namespace zpq {
static thread_local std::string g_last_error;
void set_last_error(const std::string& s) { g_last_error = s; }
}  // namespace zpq

using namespace zpq;

#define ZPQ_TRY try {
#define ZPQ_CATCH                                                        \
  }                                                                      \
  catch (const Failure& f) { set_last_error(f.what()); return f.code; } \
  catch (const std::bad_alloc&) { set_last_error("Out of memory"); return ZPQ_E_NOMEM; } \
  catch (const std::exception& ex) { set_last_error(ex.what()); return ZPQ_E_DEVICE; }

extern "C" {

const char* zpq_last_error(void) { return g_last_error.c_str(); }
const char* zpq_version(void) { return "zpaq_amd 0.1 (ZPAQ level 2, libzpaq 7.15 compatible, gfx950)"; }

int zpq_init(int device) { ZPQ_TRY engine_init(device); return ZPQ_OK; ZPQ_CATCH }
int zpq_device_count(void) { return engine_device_count(); }
void zpq_shard_range(uint64_t n, uint32_t parts, uint32_t k, uint64_t* lo, uint64_t* hi) { engine_shard_range(n, parts ? parts : 1, k, lo, hi); }
void zpq_shutdown(void) { try { engine_shutdown(); } catch (...) {} }
int zpq_set_state_budget(uint64_t bytes) { engine_set_budget(bytes); return ZPQ_OK; }
int zpq_set_kernel(int which) { if (which < 0 || which > 6) return ZPQ_E_ARG; engine_set_kernel(which); return ZPQ_OK; }

int zpq_plan_create(const uint8_t* header, size_t hlen, zpq_plan** out) {
  ZPQ_TRY
  if (!out) fail(ZPQ_E_ARG, "null out");
  *out = plan_from_header(header, hlen);
  return ZPQ_OK;
  ZPQ_CATCH
}
void zpq_plan_destroy(zpq_plan* p) { if (p) { engine_plan_release(p); delete p; } }
int zpq_plan_ncomp(const zpq_plan* p) { return p ? (int)p->hdr().n : 0; }
double zpq_plan_memory(const zpq_plan* p) { return p ? p->memory : 0; }
uint64_t zpq_plan_state_bytes(const zpq_plan* p) { return p ? p->hdr().arena_bytes : 0; }
double zpq_plan_algo_bytes_per_byte(const zpq_plan* p) { return p ? p->algo_bytes : 0; }

int zpq_plan_spec_source(const zpq_plan* p, char* src, size_t cap, size_t* len, char key41[41]) {
  ZPQ_TRY
  if (!p) fail(ZPQ_E_ARG, "null plan");
  std::string source, key, why;
  const int variant = spec_variant_forced() > 0 ? spec_variant_forced() : 0;   // ZPAQ_AMD_SPEC_WAVES selects the shape
  if (!spec_source_and_key(*p, variant, source, key, why)) fail(ZPQ_E_UNSUPPORTED, why);
  if (len) *len = source.size();
  if (key41) { memcpy(key41, key.c_str(), 40); key41[40] = 0; }
  if (source.size() + 1 > cap) fail(ZPQ_E_OVERFLOW, "source buffer too small");
  memcpy(src, source.c_str(), source.size() + 1);
  return ZPQ_OK;
  ZPQ_CATCH
}

int zpq_plan_spec_dual_source(const zpq_plan* p, char* src, size_t cap, size_t* len, char key41[41]) {
  ZPQ_TRY
  if (!p) fail(ZPQ_E_ARG, "null plan");
  std::string source, key, why;
  if (!spec_source_and_key(*p, 2, source, key, why)) fail(ZPQ_E_UNSUPPORTED, why);
  if (len) *len = source.size();
  if (key41) { memcpy(key41, key.c_str(), 40); key41[40] = 0; }
  if (source.size() + 1 > cap) fail(ZPQ_E_OVERFLOW, "source buffer too small");
  memcpy(src, source.c_str(), source.size() + 1);
  return ZPQ_OK;
  ZPQ_CATCH
}

int zpq_plan_spec_team_source(const zpq_plan* p, char* src, size_t cap, size_t* len, char key41[41]) {
  ZPQ_TRY
  if (!p) fail(ZPQ_E_ARG, "null plan");
  std::string source, key, why;
  if (!spec_source_and_key(*p, 3, source, key, why)) fail(ZPQ_E_UNSUPPORTED, why);
  if (len) *len = source.size();
  if (key41) { memcpy(key41, key.c_str(), 40); key41[40] = 0; }
  if (source.size() + 1 > cap) fail(ZPQ_E_OVERFLOW, "source buffer too small");
  memcpy(src, source.c_str(), source.size() + 1);
  return ZPQ_OK;
  ZPQ_CATCH
}

int zpq_plan_kernel_kind(zpq_plan* p, char* note, size_t cap) { return zpq_plan_kernel_kind2(p, 0, note, cap); }

int zpq_plan_kernel_kind2(zpq_plan* p, int decode, char* note, size_t cap) { return zpq_plan_kernel_kind4(p, decode, 0, 0, note, cap); }
int zpq_plan_kernel_kind3(zpq_plan* p, int decode, uint32_t nblocks, char* note, size_t cap) { return zpq_plan_kernel_kind4(p, decode, nblocks, 0, note, cap); }

int zpq_plan_kernel_kind4(zpq_plan* p, int decode, uint32_t nblocks, uint32_t block_bytes, char* note, size_t cap) {
  try {
    std::string n;
    const int k = engine_plan_kernel_kind(p, n, decode != 0, nblocks, block_bytes);
    if (note && cap) { strncpy(note, n.c_str(), cap - 1); note[cap - 1] = 0; }
    return k;
  } catch (const Failure& f) { set_last_error(f.what()); return -f.code; }
  catch (const std::exception& ex) { set_last_error(ex.what()); return -ZPQ_E_DEVICE; }
}

size_t zpq_plan_spec_jit(const zpq_plan* p, char* log, size_t cap) {
  try {
    std::string l;
    const size_t n = p ? spec_jit_compile_only(*p, spec_variant_forced() > 0 ? spec_variant_forced() : 0, l) : 0;
    if (log && cap) { strncpy(log, l.c_str(), cap - 1); log[cap - 1] = 0; }
    return n;
  } catch (const std::exception& ex) {
    if (log && cap) { strncpy(log, ex.what(), cap - 1); log[cap - 1] = 0; }
    return 0;
  }
}

size_t zpq_plan_spec_dual_jit(const zpq_plan* p, char* log, size_t cap) {
  try {
    std::string l;
    const size_t n = p ? spec_jit_compile_only(*p, 2, l) : 0;
    if (log && cap) { strncpy(log, l.c_str(), cap - 1); log[cap - 1] = 0; }
    return n;
  } catch (const std::exception& ex) {
    if (log && cap) { strncpy(log, ex.what(), cap - 1); log[cap - 1] = 0; }
    return 0;
  }
}

size_t zpq_plan_spec_team_jit(const zpq_plan* p, char* log, size_t cap) {
  try {
    std::string l;
    const size_t n = p ? spec_jit_compile_only(*p, 3, l) : 0;
    if (log && cap) { strncpy(log, l.c_str(), cap - 1); log[cap - 1] = 0; }
    return n;
  } catch (const std::exception& ex) {
    if (log && cap) { strncpy(log, ex.what(), cap - 1); log[cap - 1] = 0; }
    return 0;
  }
}

int zpq_pcomp_is_translated(const uint8_t* code, size_t codelen, int ph, int pm) {
  return code && pcomp_is_translated(code, codelen, ph, pm) ? 1 : 0;
}

int zpq_precompile(const zpq_plan* const* plans, size_t n, int decode, int threads) {
  try {
    if (!plans && n) fail(ZPQ_E_ARG, "null plans");
    std::vector<const zpq_plan*> v(plans, plans + n);
    const int forced = spec_variant_forced();
    std::string log;
    const int done = spec_precompile(v, decode == 0, forced > 0 ? forced : 0, (int)std::min<size_t>(n, 1u << 20),
                                     threads > 0 ? threads : engine_jit_threads(), &log);
    if (!log.empty()) set_last_error(log);
    return done;
  } catch (const Failure& f) { set_last_error(f.what()); return -f.code; }
  catch (const std::exception& ex) { set_last_error(ex.what()); return -ZPQ_E_DEVICE; }
}

int zpq_encoder_variants(const zpq_plan* const* plans, const uint32_t* blocks, const uint32_t* longest, uint32_t nchains,
                         int cus, int xcds, int persist_expected, int32_t* variants) {
  ZPQ_TRY
  if (!plans || !blocks || !longest || !variants || cus <= 0 || xcds <= 0) fail(ZPQ_E_ARG, "null argument or empty device");
  std::vector<ChainLoad> chains;
  for (uint32_t i = 0; i < nchains; ++i) {
    if (!plans[i]) fail(ZPQ_E_ARG, "null plan");
    chains.push_back(ChainLoad{plans[i], blocks[i], longest[i]});
  }
  const std::vector<int> v = encoder_variants(DeviceShape{cus, xcds}, launch_knobs(), persist_expected != 0, chains);
  std::copy(v.begin(), v.end(), variants);
  return ZPQ_OK;
  ZPQ_CATCH
}

const uint8_t* zpq_plan_blob(const zpq_plan* p, size_t* len) {
  if (len) *len = p ? p->blob.size() : 0;
  return p ? p->blob.data() : nullptr;
}

int zpq_plan_pipe_source(const zpq_plan* p, char* src, size_t cap, size_t* len, char key41[41]) {
  return zpq_plan_pipe_source_opts(p, 0, 0, 0, src, cap, len, key41);
}

static PipeOptions opts_of(int mode, int chunk, int group) {     // mode: a variant number of pipe_options (0, 1, 2)
  PipeOptions o = pipe_options(mode);
  if (chunk) o.chunk = chunk;
  o.group = group;
  return o;
}

int zpq_plan_pipe_source_opts(const zpq_plan* p, int mode, int chunk, int group, char* src, size_t cap, size_t* len, char key41[41]) {
  ZPQ_TRY
  if (!p) fail(ZPQ_E_ARG, "null plan");
  std::string source, key, why;
  if (!pipe_source_and_key(*p, opts_of(mode, chunk, group), source, key, why)) fail(ZPQ_E_UNSUPPORTED, why);
  if (len) *len = source.size();
  if (key41) { memcpy(key41, key.c_str(), 40); key41[40] = 0; }
  if (source.size() + 1 > cap) fail(ZPQ_E_OVERFLOW, "source buffer too small");
  memcpy(src, source.c_str(), source.size() + 1);
  return ZPQ_OK;
  ZPQ_CATCH
}

int zpq_pcomp_source(const uint8_t* code, size_t codelen, int ph, int pm, char* src, size_t cap, size_t* len, char key41[41]) {
  ZPQ_TRY
  std::string source, key, why;
  if (!pcomp_source_and_key(code, codelen, ph, pm, source, key, why)) fail(ZPQ_E_UNSUPPORTED, why);
  if (len) *len = source.size();
  if (key41) { memcpy(key41, key.c_str(), 40); key41[40] = 0; }
  if (source.size() + 1 > cap) fail(ZPQ_E_OVERFLOW, "source buffer too small");
  memcpy(src, source.c_str(), source.size() + 1);
  return ZPQ_OK;
  ZPQ_CATCH
}

int zpq_plan_pipe_layout(const zpq_plan* p, uint64_t out[16]) { return zpq_plan_pipe_layout_opts(p, 0, 0, 0, out); }

int zpq_plan_pipe_layout_opts(const zpq_plan* p, int mode, int chunk, int group, uint64_t out[16]) {
  ZPQ_TRY
  if (!p || !out) fail(ZPQ_E_ARG, "null argument");
  PipeLayout L;
  std::string why;
  if (!pipe_layout(*p, opts_of(mode, chunk, group), L, why)) fail(ZPQ_E_UNSUPPORTED, why);
  memset(out, 0, 16 * sizeof(uint64_t));
  out[0] = L.group_bytes; out[1] = (uint64_t)L.S; out[2] = (uint64_t)L.C; out[3] = L.light.size();
  out[4] = L.icm.size(); out[5] = L.isse.size(); out[6] = (uint64_t)L.mix_waves_per_group();
  out[7] = (uint64_t)L.hcomp_lanes; out[8] = (uint64_t)L.coder_level; out[9] = (uint64_t)L.G; out[10] = L.rows.size();
  out[11] = (uint64_t)L.mix_threads(); out[12] = (uint64_t)L.G; out[13] = (uint64_t)L.light_threads();
  // the persistent launch (0: the chain cannot be packed): workgroups per group, wavefronts per workgroup | progress counters per group << 16
  out[14] = L.persist_ok ? (uint64_t)L.ps_wpg : 0; out[15] = (uint64_t)L.ps_waves | (uint64_t)L.ps_nunit << 16;
  return ZPQ_OK;
  ZPQ_CATCH
}

const char* zpq_spec_cache_dir(void) { static std::string s; s = spec_cache_dir(); return s.c_str(); }
const char* zpq_spec_include_dir(void) { static std::string s; s = spec_include_dir(); return s.c_str(); }

int zpq_encode_batch(const zpq_plan* const* plans, const uint8_t* const* in, const uint32_t* in_len,
                     uint32_t nblocks, uint8_t* const* out, const uint32_t* out_cap, uint32_t* out_len,
                     int32_t* status) {
  ZPQ_TRY
  std::vector<HostBlock> hb(nblocks);
  for (uint32_t b = 0; b < nblocks; ++b) {
    if (!plans[b] || plans[b]->hdr().n == 0) fail(ZPQ_E_ARG, "encode_batch needs a modelled plan (n > 0)");
    hb[b] = HostBlock{plans[b], nullptr, 0, in[b], in_len[b], out[b], out_cap[b]};
  }
  std::vector<BlockResult> res;
  engine_code_host(false, hb, res);
  int worst = ZPQ_OK;
  for (uint32_t b = 0; b < nblocks; ++b) {
    if (out_len) out_len[b] = res[b].out_len;
    if (status) status[b] = res[b].status;
    if (res[b].status && !worst) worst = res[b].status;
  }
  if (worst) set_last_error("one or more blocks failed; see status[]");
  return worst;
  ZPQ_CATCH
}

int zpq_decode_batch(const zpq_plan* const* plans, const uint8_t* const* in, const uint32_t* in_len,
                     uint32_t nblocks, uint8_t* const* out, const uint32_t* max_out, uint32_t* out_len,
                     uint32_t* consumed, int32_t* status) {
  ZPQ_TRY
  std::vector<HostBlock> hb(nblocks);
  for (uint32_t b = 0; b < nblocks; ++b) {
    if (!plans[b] || plans[b]->hdr().n == 0) fail(ZPQ_E_ARG, "decode_batch needs a modelled plan (n > 0)");
    hb[b] = HostBlock{plans[b], nullptr, 0, in[b], in_len[b], out[b], max_out[b]};
  }
  std::vector<BlockResult> res;
  engine_code_host(true, hb, res);
  int worst = ZPQ_OK;
  for (uint32_t b = 0; b < nblocks; ++b) {
    if (out_len) out_len[b] = res[b].out_len;
    if (consumed) consumed[b] = res[b].consumed;
    if (status) status[b] = res[b].status;
    if (res[b].status && !worst) worst = res[b].status;
  }
  if (worst) set_last_error("one or more blocks failed; see status[]");
  return worst;
  ZPQ_CATCH
}

int zpq_encode_device(const zpq_plan* plan, const void* d_in, const uint64_t* in_off, const uint32_t* in_len,
                      uint32_t nblocks, void* d_out, const uint64_t* out_off, const uint32_t* out_cap,
                      zpq_block_result* d_res, void* stream, int timed) {
  ZPQ_TRY
  if (!plan || plan->hdr().n == 0) fail(ZPQ_E_ARG, "needs a modelled plan");
  engine_code_device(false, &plan, true, d_in, in_off, in_len, nblocks, d_out, out_off, out_cap, (BlockResult*)d_res,
                     stream, timed != 0);
  return ZPQ_OK;
  ZPQ_CATCH
}

int zpq_decode_device(const zpq_plan* plan, const void* d_in, const uint64_t* in_off, const uint32_t* in_len,
                      uint32_t nblocks, void* d_out, const uint64_t* out_off, const uint32_t* max_out,
                      zpq_block_result* d_res, void* stream, int timed) {
  ZPQ_TRY
  if (!plan || plan->hdr().n == 0) fail(ZPQ_E_ARG, "needs a modelled plan");
  engine_code_device(true, &plan, true, d_in, in_off, in_len, nblocks, d_out, out_off, max_out, (BlockResult*)d_res,
                     stream, timed != 0);
  return ZPQ_OK;
  ZPQ_CATCH
}

int zpq_code_device_multi(int decode, const zpq_plan* const* plans, const void* d_in, const uint64_t* in_off,
                          const uint32_t* in_len, uint32_t nblocks, void* d_out, const uint64_t* out_off,
                          const uint32_t* cap, zpq_block_result* d_res, void* stream, int timed) {
  ZPQ_TRY
  for (uint32_t b = 0; b < nblocks; ++b)
    if (!plans[b] || plans[b]->hdr().n == 0) fail(ZPQ_E_ARG, "needs modelled plans");
  engine_code_device(decode != 0, plans, false, d_in, in_off, in_len, nblocks, d_out, out_off, cap, (BlockResult*)d_res,
                     stream, timed != 0);
  return ZPQ_OK;
  ZPQ_CATCH
}

int zpq_engine_count(void) { return engine_count(); }
int zpq_last_persistent(void) { return engine_last_persistent() ? 1 : 0; }
double zpq_last_persist_abort_ms(void) { return engine_last_persist_abort_ms(); }

int zpq_last_timing(float* init_ms, float* code_ms, uint32_t* blocks) {
  Timing t = engine_last_timing();
  if (init_ms) *init_ms = t.init_ms;
  if (code_ms) *code_ms = t.code_ms;
  if (blocks) *blocks = t.blocks;
  return ZPQ_OK;
}

int zpq_selftest(int32_t out8[8]) { ZPQ_TRY return engine_selftest(out8); ZPQ_CATCH }

// ------------------------------------------------------------ block drop-ins
int zpq_compress_blocks(const char* method, uint8_t* const* in, const uint32_t* in_len, uint32_t nblocks,
                        const char* const* filename, const char* const* comment, int dosha1,
                        uint8_t* const* out, const uint64_t* out_cap, uint64_t* out_len) {
  ZPQ_TRY
  std::vector<BlockInput> inputs(nblocks);
  for (uint32_t b = 0; b < nblocks; ++b)
    inputs[b] = BlockInput{in[b], in_len[b], filename ? filename[b] : nullptr, comment ? comment[b] : nullptr};
  std::vector<std::vector<U8>> archives;
  compress_blocks(method, inputs, dosha1 != 0, archives);
  int rc = ZPQ_OK;
  for (uint32_t b = 0; b < nblocks; ++b) {
    if (out_len) out_len[b] = archives[b].size();
    if (out && out[b] && out_cap && out_cap[b] >= archives[b].size())
      memcpy(out[b], archives[b].data(), archives[b].size());
    else { rc = ZPQ_E_OVERFLOW; set_last_error("output buffer too small"); }
  }
  return rc;
  ZPQ_CATCH
}

int zpq_decompress(const uint8_t* archive, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* out_len) {
  ZPQ_TRY
  U64 total = 0;
  bool overflow = false;
  decode_archive(archive, (size_t)n, [&](const U8* p, size_t len) {
    if (out && total + len <= cap) { if (len) memcpy(out + total, p, len); }      // (an empty segment's data pointer may be null)
    else overflow = true;
    total += len;
  });
  if (out_len) *out_len = total;
  if (overflow) { set_last_error("output buffer too small"); return ZPQ_E_OVERFLOW; }
  return ZPQ_OK;
  ZPQ_CATCH
}

// ------------------------------------------------------------- host pieces
void zpq_sha1(const uint8_t* in, uint64_t n, uint8_t out20[20]) {
  Sha1 s; s.update(in, (size_t)n); memcpy(out20, s.result(), 20);
}
void zpq_sha1_force_portable(int yes) { sha1_force_portable(yes != 0); }
void zpq_set_pcomp_step_limit(uint64_t steps) { postproc_set_step_limit(steps); }

void zpq_e8e9(uint8_t* data, uint32_t n) { e8e9_forward(data, n); }

// the host's suffix sorter (SA-IS, host/preproc.cpp): what the library uses when the device is not asked
int zpq_suffix_array_host(const uint8_t* in, uint32_t n, uint32_t* out) {
  ZPQ_TRY
  const std::vector<U32> sa = suffix_array(in, n);
  if (n) memcpy(out, sa.data(), 4ull * n);
  return ZPQ_OK;
  ZPQ_CATCH
}

// Suffix arrays of n host buffers, built on the device in one call (device/sa_kernels.hip); out[i] receives len[i] entries.
int zpq_suffix_arrays_device(const uint8_t* const* in, const uint32_t* len, uint32_t n, uint32_t* const* out) {
  ZPQ_TRY
  std::vector<std::pair<const U8*, U32>> blk;
  for (uint32_t i = 0; i < n; ++i) blk.push_back({in[i], len[i]});
  std::vector<std::vector<U32>> sa;
  std::string note;
  if (!engine_suffix_arrays(blk, sa, note)) fail(ZPQ_E_UNSUPPORTED, "suffix arrays on the device unavailable: " + note);
  for (uint32_t i = 0; i < n; ++i) if (len[i]) memcpy(out[i], sa[i].data(), 4ull * len[i]);
  return ZPQ_OK;
  ZPQ_CATCH
}

// One buffer of any length below 2^31 through the wide sorter (device/sa_wide_kernel.h); out receives n entries.
int zpq_suffix_array_device_wide(const uint8_t* in, uint32_t n, uint32_t* out) {
  ZPQ_TRY
  if ((!in || !out) && n) fail(ZPQ_E_ARG, "null argument");
  if (n >= (1u << 31)) fail(ZPQ_E_UNSUPPORTED, "wide suffix sort on the device unavailable: block outside the wide sorter's range");
  if (engine_device_count() <= 0) fail(ZPQ_E_UNSUPPORTED, "wide suffix sort on the device unavailable: no device");
  SortOut so;
  std::string note;
  if (!engine_sort_wide(SortJob{in, n, 0u, 0u, 0u, 0u, 0u}, so, note, true)) fail(ZPQ_E_UNSUPPORTED, "wide suffix sort on the device unavailable: " + note);
  if (n) memcpy(out, so.sa.data(), 4ull * n);
  return ZPQ_OK;
  ZPQ_CATCH
}
uint32_t zpq_last_wide_sort_blocks(void) { return last_wide_sort_blocks(); }
uint32_t zpq_last_wide_sort_rounds(void) { return engine_last_wide_sort_rounds(); }

uint32_t zpq_last_wide_parse_blocks(void) { return last_wide_parse_blocks(); }
void zpq_last_wide_parse_pieces(uint32_t out4[4]) { if (out4) engine_last_wide_parse_pieces(out4); }

// What a wide call holds on the device: out2[0] the sort alone, out2[1] the sort with the parse and the coder's arrays
int zpq_wide_stage_bytes(const char* xmethod, uint32_t n, uint64_t out2[2]) {
  ZPQ_TRY
  if (!xmethod || !out2) fail(ZPQ_E_ARG, "null argument");
  int args[9];
  (void)make_config(xmethod, args);
  if (!preprocess_needs_suffix_array(args)) fail(ZPQ_E_UNSUPPORTED, "the method's pre-processor does not sort suffixes");
  if (n >= (1u << 31)) fail(ZPQ_E_UNSUPPORTED, "block outside the wide sorter's range");
  U64 sums[2];
  engine_wide_stage_bytes(sort_job(nullptr, n, args), sums);
  out2[0] = sums[0];
  out2[1] = sums[1];
  return ZPQ_OK;
  ZPQ_CATCH
}

// E8E9 applied in place for the length of a stage call: taken back on every failure exit, as in zpq_preprocess_blocks_device
namespace {
struct Unfilter {
  uint8_t* data; uint32_t n; bool done = false, keep = false;
  ~Unfilter() { if (done && !keep) e8e9_inverse(data, n); }
};
}  // namespace

// The wide stage's parse on its own: E8E9 as the method says, the wide sort, the parse in pieces (device/lz77_wide_kernel.h).
// The list in zpq_lz77_tokens_host's layout; *count always, nothing is written when cap is short.
int zpq_lz77_parse_device_wide(const char* xmethod, uint8_t* data, uint32_t n, uint32_t* tokens4, size_t cap, size_t* count) {
  ZPQ_TRY
  if (!xmethod || (!data && n) || !count || (!tokens4 && cap)) fail(ZPQ_E_ARG, "null argument");
  *count = 0;
  int args[9];
  (void)make_config(xmethod, args);
  const int level = args[1] & 3;
  if (!preprocess_needs_suffix_array(args) || level < 1 || level > 2)
    fail(ZPQ_E_UNSUPPORTED, "wide parse on the device unavailable: the method's LZ77 does not search a suffix array");
  if (n >= (1u << 31)) fail(ZPQ_E_UNSUPPORTED, "wide parse on the device unavailable: block outside the wide sorter's range");
  if (engine_device_count() <= 0) fail(ZPQ_E_UNSUPPORTED, "wide parse on the device unavailable: no device");
  if (n == 0) return ZPQ_OK;
  Unfilter guard{data, n};
  if (args[1] > 4) { e8e9_forward(data, n); guard.done = true; }
  SortOut so;
  std::string note;
  if (!engine_sort_wide(sort_job(data, n, args), so, note, false, 0, true)) fail(ZPQ_E_UNSUPPORTED, "wide parse on the device unavailable: " + note);
  if (!so.parsed) fail(ZPQ_E_UNSUPPORTED, "wide parse on the device unavailable: " + note);
  *count = so.toks.size();
  if (so.toks.size() > cap) fail(ZPQ_E_OVERFLOW, "token buffer too small");
  if (!so.toks.empty()) memcpy(tokens4, so.toks.data(), so.toks.size() * sizeof(LzToken));
  guard.keep = true;
  return ZPQ_OK;
  ZPQ_CATCH
}

// What zpq_preprocess_block makes of one buffer, the sort by the wide sorter: a BWT method's last column is emitted on the
// device; an LZ77 method that sorts suffixes is parsed by the host with the device's array, or -- ZPAQ_AMD_DEVICE_PARSE_WIDE=1, or
// unset and lz_wide_parse_pays -- on the device in pieces, its codes written there too as ZPAQ_AMD_DEVICE_CODES says.  E8E9 is
// applied in place and taken back on every failure exit, as in zpq_preprocess_blocks_device.
int zpq_preprocess_block_device_wide(const char* xmethod, uint8_t* data, uint32_t n, uint8_t* out, size_t cap, size_t* len) {
  ZPQ_TRY
  if (!xmethod || (!data && n) || !len) fail(ZPQ_E_ARG, "null argument");
  int args[9];
  (void)make_config(xmethod, args);
  if (!preprocess_needs_suffix_array(args)) fail(ZPQ_E_UNSUPPORTED, "the method's pre-processor does not sort suffixes");
  if (n >= (1u << 31)) fail(ZPQ_E_UNSUPPORTED, "pre-processing on the device unavailable: block outside the wide sorter's range");
  if (engine_device_count() <= 0) fail(ZPQ_E_UNSUPPORTED, "pre-processing on the device unavailable: no device");
  Unfilter guard{data, n};
  if (args[1] > 4) { e8e9_forward(data, n); guard.done = true; }
  std::vector<U8> pre;
  if (n == 0) (void)preprocess_block(data, 0, args, pre, nullptr, true);
  else {
    SortOut so;
    std::string note;
    const int mode = device_parse_wide_mode();
    const bool parse_there = (args[1] & 3) != 3 && (mode == 1 || (mode == 2 && n >= (1u << 24) && lz_wide_parse_pays(n)));
    if (!engine_sort_wide(sort_job(data, n, args), so, note, false, parse_there ? device_codes_mode() : -1))
      fail(ZPQ_E_UNSUPPORTED, "pre-processing on the device unavailable: " + note);
    if ((args[1] & 3) == 3) pre.swap(so.bwt);
    else if (so.parsed && so.coded) pre.swap(so.codes);
    else if (so.parsed) lz77_serialize(data, n, args, so.toks.data(), so.toks.size(), pre);
    else (void)preprocess_block(data, n, args, pre, so.sa.data(), true);
  }
  *len = pre.size();                                      // (the size is reported also when the buffer is too small)
  if (pre.size() > cap) fail(ZPQ_E_OVERFLOW, "output buffer too small");
  if (!pre.empty()) memcpy(out, pre.data(), pre.size());
  guard.keep = true;
  return ZPQ_OK;
  ZPQ_CATCH
}

int zpq_expand_method(const char* method, const uint8_t* data, uint32_t n, char* out, size_t cap) {
  ZPQ_TRY
  const std::string m = expand_method(method ? method : "", data, n);
  if (m.size() + 1 > cap) fail(ZPQ_E_OVERFLOW, "method buffer too small");
  memcpy(out, m.c_str(), m.size() + 1);
  return ZPQ_OK;
  ZPQ_CATCH
}

static int copy_assembled(const Assembled& as, uint8_t* hcomp, size_t hcap, size_t* hlen, uint8_t* pcomp,
                          size_t pcap, size_t* plen) {
  if (hlen) *hlen = as.hcomp.size();
  if (plen) *plen = as.pcomp.size();
  if (as.hcomp.size() > hcap || as.pcomp.size() > pcap) fail(ZPQ_E_OVERFLOW, "header buffer too small");
  if (hcomp) memcpy(hcomp, as.hcomp.data(), as.hcomp.size());
  if (pcomp && !as.pcomp.empty()) memcpy(pcomp, as.pcomp.data(), as.pcomp.size());
  return ZPQ_OK;
}

int zpq_method_to_header(const char* xmethod, int* args9, uint8_t* hcomp, size_t hcap, size_t* hlen,
                         uint8_t* pcomp, size_t pcap, size_t* plen) {
  ZPQ_TRY
  int args[9];
  const std::string cfg = make_config(xmethod ? xmethod : "", args);
  if (args9) memcpy(args9, args, sizeof(args));
  return copy_assembled(assemble(cfg.c_str(), args), hcomp, hcap, hlen, pcomp, pcap, plen);
  ZPQ_CATCH
}

// the stored header of one of the reference's three built-in models (Compressor::startBlock(int level), libzpaq.cpp:2793-2839:
// min.cfg, mid.cfg, max.cfg) -- what a block coded at that level carries; the batch entry points take it like any other header
int zpq_builtin_model_header(int level, uint8_t* hcomp, size_t hcap, size_t* hlen) {
  ZPQ_TRY
  const std::vector<U8> h = builtin_model(level);
  if (h.empty()) fail(ZPQ_E_ARG, "built-in models are levels 1, 2 and 3");
  if (hlen) *hlen = h.size();
  if (h.size() > hcap || !hcomp) fail(ZPQ_E_OVERFLOW, "header buffer too small");
  memcpy(hcomp, h.data(), h.size());
  return ZPQ_OK;
  ZPQ_CATCH
}

int zpq_assemble(const char* config, const int* args9, uint8_t* hcomp, size_t hcap, size_t* hlen,
                 uint8_t* pcomp, size_t pcap, size_t* plen) {
  ZPQ_TRY
  return copy_assembled(assemble(config, args9), hcomp, hcap, hlen, pcomp, pcap, plen);
  ZPQ_CATCH
}

int zpq_preprocess_block(const char* xmethod, uint8_t* data, uint32_t n, uint8_t* out, size_t cap, size_t* len) {
  return zpq_preprocess_block_sa(xmethod, data, n, nullptr, out, cap, len);
}

// ... with the block's suffix array supplied by the caller (what zpq_compress_blocks does with the arrays the device built
// for a whole batch): for a method with E8E9 the caller applies zpq_e8e9 first -- the sort is over the filtered bytes --
// and says so with sa != null (then the call does not filter again)
int zpq_preprocess_block_sa(const char* xmethod, uint8_t* data, uint32_t n, const uint32_t* sa, uint8_t* out, size_t cap, size_t* len) {
  ZPQ_TRY
  if (!xmethod || (!data && n) || !len) fail(ZPQ_E_ARG, "null argument");
  int args[9];
  (void)make_config(xmethod, args);
  std::vector<U8> pre;
  const bool made = preprocess_block(data, n, args, pre, sa, sa != nullptr);
  if (!made) pre.assign(data, data + n);
  *len = pre.size();
  if (pre.size() > cap) fail(ZPQ_E_OVERFLOW, "output buffer too small");
  if (!pre.empty()) memcpy(out, pre.data(), pre.size());
  return ZPQ_OK;
  ZPQ_CATCH
}

// ---- the LZ77 parse (through a suffix array or LZBuffer's hash table) as a token list (host/common.hpp LzToken: i, off, len, blit) ----
static void lz_args(const char* xmethod, int args[9]) {
  if (!xmethod) fail(ZPQ_E_ARG, "null argument");
  (void)make_config(xmethod, args);
  const int level = args[1] & 3;
  if (args[1] < 1 || args[1] > 7 || level < 1 || level > 2) fail(ZPQ_E_ARG, "not an LZ77 method");
}

// The host's parse of one block (data is E8E9-filtered in place first when the method says so).
int zpq_lz77_tokens_host(const char* xmethod, uint8_t* data, uint32_t n, uint32_t* tokens4, size_t cap, size_t* count) {
  ZPQ_TRY
  if ((!data && n) || !count || (!tokens4 && cap)) fail(ZPQ_E_ARG, "null argument");
  int args[9];
  lz_args(xmethod, args);
  if (args[1] > 4) e8e9_forward(data, n);
  std::vector<LzToken> toks;
  lz77_host_tokens(data, n, args, nullptr, toks);
  *count = toks.size();
  if (toks.size() > cap) fail(ZPQ_E_OVERFLOW, "token buffer too small");
  if (!toks.empty()) memcpy(tokens4, toks.data(), toks.size() * sizeof(LzToken));
  return ZPQ_OK;
  ZPQ_CATCH
}

// The coded stream of a token list (what zpq_preprocess_block returns for the same block and the host's list); `data` as the
// parse saw it (E8E9 already applied).
int zpq_lz77_serialize(const char* xmethod, const uint8_t* data, uint32_t n, const uint32_t* tokens4, size_t ntok, uint8_t* out, size_t cap, size_t* len) {
  ZPQ_TRY
  if ((!data && n) || (!tokens4 && ntok) || !len) fail(ZPQ_E_ARG, "null argument");
  int args[9];
  lz_args(xmethod, args);
  std::vector<U8> pre;
  lz77_serialize(data, n, args, (const LzToken*)tokens4, ntok, pre);
  *len = pre.size();
  if (pre.size() > cap) fail(ZPQ_E_OVERFLOW, "output buffer too small");
  if (!pre.empty()) memcpy(out, pre.data(), pre.size());
  return ZPQ_OK;
  ZPQ_CATCH
}

// What zpq_preprocess_block makes, for n host buffers in one call with the sort, the LZ77 parse and the BWT on the device
// (device/sa_kernels.hip, device/lz77_kernel.h), or the LZ77 parse through the hash table (device/lz77_hash_kernel.h); only for
// methods whose pre-processor sorts or is such an LZ77.  E8E9 is applied in place.
int zpq_preprocess_blocks_device(const char* xmethod, uint8_t* const* data, const uint32_t* len, uint32_t n, uint8_t* const* out, const size_t* cap,
                                 size_t* outlen) {
  ZPQ_TRY
  if (!xmethod || (n && (!data || !len || !out || !cap || !outlen))) fail(ZPQ_E_ARG, "null argument");
  int args[9];
  (void)make_config(xmethod, args);
  const bool hashed = preprocess_is_hash_lz77(args);
  if (!hashed && !preprocess_needs_suffix_array(args)) fail(ZPQ_E_ARG, "the method's pre-processor neither sorts nor parses");
  // E8E9 rewrites the caller's buffers in place (as the reference rewrites its input).  They keep the filter only when the call
  // succeeds: on EVERY failure exit -- the device declines, something throws between the first filtered buffer and the last
  // copied output, an output buffer is too small -- the buffers filtered so far go back as they came, so that a caller
  // that falls back to zpq_preprocess_block (or calls again with larger buffers) never filters a block twice.
  struct Unfilter {
    uint8_t* const* data; const uint32_t* len; uint32_t done = 0; bool keep = false;
    ~Unfilter() { if (!keep) for (uint32_t i = 0; i < done; ++i) e8e9_inverse(data[i], len[i]); }
  } guard{data, len};
  std::vector<SortJob> jobs;
  for (uint32_t i = 0; i < n; ++i) {
    if (args[1] > 4) { e8e9_forward(data[i], len[i]); guard.done = i + 1; }
    jobs.push_back(hashed ? hash_job(data[i], len[i], args) : sort_job(data[i], len[i], args));
  }
  std::vector<SortOut> outs;
  std::string note;
  const int codes = device_codes_mode();
  if (!(hashed ? engine_hash_preprocess(jobs, outs, note, codes) : engine_sort_preprocess(jobs, outs, note, codes))) fail(ZPQ_E_UNSUPPORTED, "pre-processing on the device unavailable: " + note);
  std::vector<std::vector<U8>> pres(n);
  bool fits = true;
  for (uint32_t i = 0; i < n; ++i) {
    std::vector<U8>& pre = pres[i];
    if (len[i] == 0) (void)preprocess_block(data[i], 0, args, pre, nullptr, true);
    else if (jobs[i].kind == 3) pre.swap(outs[i].bwt);
    else if (outs[i].coded) pre.swap(outs[i].codes);
    else lz77_serialize(data[i], len[i], args, outs[i].toks.data(), outs[i].toks.size(), pre);
    outlen[i] = pre.size();                               // (every size is reported, also when some buffer is too small)
    fits = fits && pre.size() <= cap[i];
  }
  if (!fits) fail(ZPQ_E_OVERFLOW, "output buffer too small");
  for (uint32_t i = 0; i < n; ++i)
    if (!pres[i].empty()) memcpy(out[i], pres[i].data(), pres[i].size());
  guard.keep = true;
  return ZPQ_OK;
  ZPQ_CATCH
}

// zpq_lz77_serialize for a batch, with the codes written on the device (device/lz77_codes_kernel.h)
int zpq_lz77_serialize_device(const char* xmethod, const uint8_t* const* data, const uint32_t* len, const uint32_t* const* tokens4, const size_t* ntok,
                              uint32_t nblocks, uint8_t* const* out, const size_t* cap, size_t* outlen) {
  ZPQ_TRY
  if (nblocks && (!data || !len || !tokens4 || !ntok || !out || !cap || !outlen)) fail(ZPQ_E_ARG, "null argument");
  int args[9];
  lz_args(xmethod, args);
  std::vector<CodeJob> jobs;
  for (uint32_t i = 0; i < nblocks; ++i) {
    if ((!data[i] && len[i]) || (!tokens4[i] && ntok[i])) fail(ZPQ_E_ARG, "null argument");
    jobs.push_back(CodeJob{data[i], len[i], (U32)(args[1] & 3), (U32)args[2], lz_offset_rb(args), (const LzToken*)tokens4[i], ntok[i]});
  }
  if (engine_device_count() <= 0) fail(ZPQ_E_UNSUPPORTED, "coding on the device unavailable: no device");
  std::vector<std::vector<U8>> pres;
  std::string note;
  const int got = engine_lz77_codes(jobs, pres, note);
  if (got < 0) fail(ZPQ_E_UNSUPPORTED, "coding on the device unavailable: " + note);
  if (got == 0) fail(ZPQ_E_DEVICE, note);
  bool fits = true;
  for (uint32_t i = 0; i < nblocks; ++i) {
    outlen[i] = pres[i].size();                           // (every size is reported, also when some buffer is too small)
    fits = fits && pres[i].size() <= cap[i];
  }
  if (!fits) fail(ZPQ_E_OVERFLOW, "output buffer too small");
  for (uint32_t i = 0; i < nblocks; ++i)
    if (!pres[i].empty()) memcpy(out[i], pres[i].data(), pres[i].size());
  return ZPQ_OK;
  ZPQ_CATCH
}

// The method's own PCOMP program over one stream (host/postproc.cpp): a segment's decoded bytes are the PP header -- 0, or
// 1 len16 program -- and the stream.
int zpq_postprocess_block(const char* xmethod, const uint8_t* stream, uint32_t len, uint8_t* out, size_t cap, size_t* outlen) {
  ZPQ_TRY
  if (!xmethod || (!stream && len) || !outlen) fail(ZPQ_E_ARG, "null argument");
  int args[9];
  const std::string cfg = make_config(xmethod, args);
  const Assembled as = assemble(cfg.c_str(), args);
  std::vector<U8> decoded, data;
  decoded.reserve(1 + as.pcomp.size() + len);
  decoded.push_back(as.pcomp.empty() ? 0 : 1);
  decoded.insert(decoded.end(), as.pcomp.begin(), as.pcomp.end());
  if (len) decoded.insert(decoded.end(), stream, stream + len);
  post_process(as.hcomp, decoded, data);
  *outlen = data.size();
  if (data.size() > cap) fail(ZPQ_E_OVERFLOW, "output buffer too small");
  if (!data.empty()) memcpy(out, data.data(), data.size());
  return ZPQ_OK;
  ZPQ_CATCH
}

// ... for a batch of streams on the device.  What the three entries below share: `wrong` is the entry's own method check (null:
// the method is its route's; else why not), `decode` its engine call over the jobs (1 done, 0 a buffer too small, -1 + note).
static int decode_streams_device(const char* xmethod, const uint8_t* const* stream, const uint32_t* len, uint32_t n, uint8_t* const* out, const size_t* cap,
                                 size_t* outlen, int32_t* status, const char* (*wrong)(const char* xmethod, const int* args),
                                 int (*decode)(const int* args, std::vector<StreamJob>& jobs, std::string& note)) {
  ZPQ_TRY
  if (!xmethod || (n && (!stream || !len || !out || !cap || !outlen || !status))) fail(ZPQ_E_ARG, "null argument");
  int args[9];
  (void)make_config(xmethod, args);
  if (const char* why = wrong(xmethod, args)) fail(ZPQ_E_UNSUPPORTED, std::string("decoding on the device unavailable: ") + why);
  std::vector<StreamJob> jobs;
  for (uint32_t i = 0; i < n; ++i) {
    if (!stream[i] && len[i]) fail(ZPQ_E_ARG, "null argument");
    outlen[i] = 0;
    status[i] = 1;
    jobs.push_back(StreamJob{stream[i], len[i], out[i], cap[i], nullptr});
  }
  if (engine_device_count() <= 0) fail(ZPQ_E_UNSUPPORTED, "decoding on the device unavailable: no device");
  std::string note;
  const int got = decode(args, jobs, note);
  if (got < 0) fail(ZPQ_E_UNSUPPORTED, "decoding on the device unavailable: " + note);
  for (uint32_t i = 0; i < n; ++i) outlen[i] = (size_t)jobs[i].out_len;       // (every size is reported, also when some buffer is too small)
  if (got == 0) fail(ZPQ_E_OVERFLOW, "output buffer too small");
  for (uint32_t i = 0; i < n; ++i) status[i] = jobs[i].status;
  return ZPQ_OK;
  ZPQ_CATCH
}

// LZ77 streams (device/lz77_decode_kernel.h)
int zpq_lz77_decode_device(const char* xmethod, const uint8_t* const* stream, const uint32_t* len, uint32_t n, uint8_t* const* out, const size_t* cap,
                           size_t* outlen, int32_t* status) {
  return decode_streams_device(xmethod, stream, len, n, out, cap, outlen, status,
      [](const char* xm, const int* args) -> const char* {
        const int level = args[1] & 3;
        return xm[0] == '0' || args[1] < 1 || args[1] > 3 || level < 1 || level > 2 ? "not an LZ77 method of level 1 or 2 without E8E9" : nullptr;
      },
      [](const int* args, std::vector<StreamJob>& jobs, std::string& note) {
        return engine_lz77_decode((U32)(args[1] & 3), lz_offset_rb(args), (U32)args[2], (U32)(args[0] + 20), jobs, note);
      });
}

uint32_t zpq_last_device_unlz_segments(void) { return last_device_unlz_segments(); }

// ... LZ77 streams parsed in pieces (device/lz77_decode_wide_kernel.h)
int zpq_lz77_decode_device_wide(const char* xmethod, const uint8_t* const* stream, const uint32_t* len, uint32_t n, uint8_t* const* out, const size_t* cap,
                                size_t* outlen, int32_t* status) {
  return decode_streams_device(xmethod, stream, len, n, out, cap, outlen, status,
      [](const char* xm, const int* args) -> const char* {
        const int level = args[1] & 3;
        return xm[0] == '0' || args[1] < 1 || args[1] > 3 || level < 1 || level > 2 ? "not an LZ77 method of level 1 or 2 without E8E9" : nullptr;
      },
      [](const int* args, std::vector<StreamJob>& jobs, std::string& note) {
        return engine_lz77_decode_wide((U32)(args[1] & 3), lz_offset_rb(args), (U32)args[2], (U32)(args[0] + 20), jobs, note);
      });
}

uint32_t zpq_last_device_unlz_wide_segments(void) { return last_device_unlz_wide_segments(); }
void zpq_last_unlz_wide_pieces(uint32_t out4[4]) { if (out4) engine_last_unlz_wide_pieces(out4); }
uint32_t zpq_last_unlz_wide_rounds(void) { return engine_last_unlz_wide_rounds(); }

// ... BWT streams (device/bwt_decode_kernel.h)
int zpq_bwt_decode_device(const char* xmethod, const uint8_t* const* stream, const uint32_t* len, uint32_t n, uint8_t* const* out, const size_t* cap,
                          size_t* outlen, int32_t* status) {
  return decode_streams_device(xmethod, stream, len, n, out, cap, outlen, status,
      [](const char* xm, const int* args) -> const char* {
        return xm[0] == '0' || args[1] != 3 || args[0] > 4 ? "not a BWT method (level 3) without E8E9 at args[0] <= 4" : nullptr;
      },
      [](const int* args, std::vector<StreamJob>& jobs, std::string& note) { return engine_bwt_decode((U32)(args[0] + 20), jobs, note); });
}

uint32_t zpq_last_device_unbwt_segments(void) { return last_device_unbwt_segments(); }

// ... BWT streams of the program at args[0] 5 .. 11, without E8E9 or behind it (device/bwt_decode_wide_kernel.h)
int zpq_bwt_decode_device_wide(const char* xmethod, const uint8_t* const* stream, const uint32_t* len, uint32_t n, uint8_t* const* out, const size_t* cap,
                               size_t* outlen, int32_t* status) {
  return decode_streams_device(xmethod, stream, len, n, out, cap, outlen, status,
      [](const char* xm, const int* args) -> const char* {
        return xm[0] == '0' || (args[1] != 3 && args[1] != 7) || args[0] < 5 || args[0] > 11 ? "not a BWT method (level 3, with or without E8E9) at args[0] 5 .. 11"
                                                                                             : nullptr;
      },
      [](const int* args, std::vector<StreamJob>& jobs, std::string& note) { return engine_bwt_decode_wide((U32)(args[0] + 20), args[1] == 7, jobs, note); });
}

// ... and streams of an E8E9 method (device/e8e9_kernel.h behind the stage's decoder)
int zpq_e8e9_decode_device(const char* xmethod, const uint8_t* const* stream, const uint32_t* len, uint32_t n, uint8_t* const* out, const size_t* cap,
                           size_t* outlen, int32_t* status) {
  return decode_streams_device(xmethod, stream, len, n, out, cap, outlen, status,
      [](const char* xm, const int* args) -> const char* {
        return xm[0] == '0' || args[1] < 4 || args[1] > 7 || (args[1] == 7 && args[0] > 4) ? "not an E8E9 method (args[1] 4 .. 7, the BWT at args[0] <= 4)" : nullptr;
      },
      [](const int* args, std::vector<StreamJob>& jobs, std::string& note) {
        return engine_e8e9_decode(args[1], lz_offset_rb(args), (U32)args[2], (U32)(args[0] + 20), jobs, note);
      });
}

uint32_t zpq_last_device_une8_segments(void) { return last_device_une8_segments(); }

// The forward filter on its own, n buffers in place (device/e8e9_forward_kernel.h)
int zpq_e8e9_device(uint8_t* const* data, const uint32_t* len, uint32_t n, uint32_t max_steps, int32_t* status) {
  ZPQ_TRY
  if ((!data || !len || !status) && n) fail(ZPQ_E_ARG, "null argument");
  for (uint32_t i = 0; i < n; ++i) {
    if (!data[i] && len[i]) fail(ZPQ_E_ARG, "null argument");
    status[i] = 1;
  }
  if (engine_device_count() <= 0) fail(ZPQ_E_UNSUPPORTED, "E8E9 filter on the device unavailable: no device");
  std::string note;
  if (!engine_e8e9_device(data, len, n, max_steps, status, note)) fail(ZPQ_E_UNSUPPORTED, "E8E9 filter on the device unavailable: " + note);
  return ZPQ_OK;
  ZPQ_CATCH
}
uint32_t zpq_last_device_e8_blocks(void) { return last_device_e8_blocks(); }

// ... streams of x.,5 / x.,6 parsed in pieces, then filtered (device/lz77_decode_wide_kernel.h, device/e8e9_kernel.h)
int zpq_e8e9_decode_device_wide(const char* xmethod, const uint8_t* const* stream, const uint32_t* len, uint32_t n, uint8_t* const* out, const size_t* cap,
                                size_t* outlen, int32_t* status) {
  return decode_streams_device(xmethod, stream, len, n, out, cap, outlen, status,
      [](const char* xm, const int* args) -> const char* {
        return xm[0] == '0' || (args[1] != 5 && args[1] != 6) || args[0] < 0 || args[0] > 11 ? "not an LZ77 method behind E8E9 (args[1] 5 or 6, args[0] 0 .. 11)"
                                                                                             : nullptr;
      },
      [](const int* args, std::vector<StreamJob>& jobs, std::string& note) {
        return engine_e8e9_decode_wide(args[1], lz_offset_rb(args), (U32)args[2], (U32)(args[0] + 20), jobs, note);
      });
}

uint32_t zpq_last_device_une8_wide_segments(void) { return last_device_une8_wide_segments(); }

// A raw PCOMP program over a batch of raw streams on the device (device/pcomp_kernel.h through engine_pcomp) ...
int zpq_pcomp_device(const uint8_t* code, size_t codelen, int ph, int pm, const uint8_t* const* stream, const uint32_t* len, uint32_t n,
                     const uint64_t* hint, uint8_t* const* out, const size_t* cap, size_t* outlen, int32_t* status) {
  ZPQ_TRY
  if (!code || !codelen || (n && (!stream || !len || !out || !cap || !outlen || !status))) fail(ZPQ_E_ARG, "null argument");
  if (ph < 0 || pm < 0 || ph > 255 || pm > 255) fail(ZPQ_E_ARG, "ph / pm outside a header byte");
  std::vector<std::vector<U8>> res(n);
  std::vector<PcompSeg> segs;
  for (uint32_t i = 0; i < n; ++i) {
    if (!stream[i] && len[i]) fail(ZPQ_E_ARG, "null argument");
    outlen[i] = 0;
    status[i] = 1;
    segs.push_back(PcompSeg{stream[i], len[i], hint ? hint[i] : 0, &res[i]});
  }
  if (engine_device_count() <= 0) fail(ZPQ_E_UNSUPPORTED, "post-processing on the device unavailable: no device");
  std::string note;
  bool handed_back = false;
  if (!engine_pcomp(code, codelen, ph, pm, segs, note, &handed_back)) {
    if (!handed_back) fail(ZPQ_E_UNSUPPORTED, "post-processing on the device unavailable: " + note);
    set_last_error(note);                 // declined: the caller runs the batch on the host
    return ZPQ_OK;
  }
  bool fits = true;
  for (uint32_t i = 0; i < n; ++i) { outlen[i] = res[i].size(); fits = fits && res[i].size() <= cap[i]; }
  if (!fits) fail(ZPQ_E_OVERFLOW, "output buffer too small");
  for (uint32_t i = 0; i < n; ++i) {
    if (!res[i].empty()) memcpy(out[i], res[i].data(), res[i].size());
    status[i] = 0;
  }
  return ZPQ_OK;
  ZPQ_CATCH
}

// ... and over one stream through the host's interpreter (host/postproc.cpp)
int zpq_pcomp_host(const uint8_t* code, size_t codelen, int ph, int pm, const uint8_t* in, uint32_t len, uint8_t* out, size_t cap, size_t* outlen) {
  ZPQ_TRY
  if (!code || (!in && len) || !outlen) fail(ZPQ_E_ARG, "null argument");
  if (ph < 0 || pm < 0 || ph > 255 || pm > 255) fail(ZPQ_E_ARG, "ph / pm outside a header byte");
  *outlen = 0;
  std::vector<U8> data;
  pcomp_interpret(code, codelen, ph, pm, in, len, data);
  *outlen = data.size();
  if (data.size() > cap) fail(ZPQ_E_OVERFLOW, "output buffer too small");
  if (!data.empty()) memcpy(out, data.data(), data.size());
  return ZPQ_OK;
  ZPQ_CATCH
}

uint32_t zpq_last_device_pcomp_segments(void) { return last_device_pcomp_segments(); }

// The archiver's fragmenting (host/fragment.cpp; on the device: device/fragment_kernel.h through engine_fragment)
void zpq_fragment_limits(int fragment, uint32_t blocksize, uint32_t* min_frag, uint32_t* max_frag) {
  if (blocksize < 13u) blocksize = 13u;
  const FragLimits l = fragment_limits(fragment, blocksize);
  if (min_frag) *min_frag = l.min_frag;
  if (max_frag) *max_frag = l.max_frag;
}

namespace {
int fragment_deliver(const std::vector<std::vector<Fragment>>& fr, uint32_t n, uint32_t* nfrag, uint32_t* size, uint32_t* hits, uint8_t* sha1,
                     uint8_t* o1, size_t cap, size_t* total) {
  size_t all = 0;
  for (uint32_t f = 0; f < n; ++f) all += fr[f].size();
  *total = all;
  if (all > cap) fail(ZPQ_E_OVERFLOW, "output arrays too small");
  if (all && (!size || !hits || !sha1 || !o1)) fail(ZPQ_E_ARG, "null argument");
  size_t k = 0;
  for (uint32_t f = 0; f < n; ++f) {
    nfrag[f] = (uint32_t)fr[f].size();
    for (const Fragment& x : fr[f]) {
      size[k] = x.size;
      hits[k] = x.hits;
      memcpy(sha1 + 20 * k, x.sha1, 20);
      memcpy(o1 + 256 * k, x.o1, 256);
      ++k;
    }
  }
  return ZPQ_OK;
}
void fragment_args(const uint8_t* const* in, const uint64_t* len, uint32_t n, uint32_t blocksize, const uint32_t* nfrag, const size_t* total) {
  if (!total || (n && (!in || !len || !nfrag))) fail(ZPQ_E_ARG, "null argument");
  if (blocksize < 13u) fail(ZPQ_E_ARG, "blocksize below 13");
  for (uint32_t f = 0; f < n; ++f) if (!in[f] && len[f]) fail(ZPQ_E_ARG, "null argument");
}
}  // namespace

int zpq_fragment_host(const uint8_t* const* in, const uint64_t* len, uint32_t n, int fragment, uint32_t blocksize, uint32_t* nfrag, uint32_t* size,
                      uint32_t* hits, uint8_t* sha1, uint8_t* o1, size_t cap, size_t* total) {
  ZPQ_TRY
  fragment_args(in, len, n, blocksize, nfrag, total);
  const FragLimits lim = fragment_limits(fragment, blocksize);
  std::vector<std::vector<Fragment>> fr(n);
  for (uint32_t f = 0; f < n; ++f) fragment_scan(in[f], len[f], lim, true, fr[f]);
  return fragment_deliver(fr, n, nfrag, size, hits, sha1, o1, cap, total);
  ZPQ_CATCH
}

int zpq_fragment_device(const uint8_t* const* in, const uint64_t* len, uint32_t n, int fragment, uint32_t blocksize, uint32_t* nfrag, uint32_t* size,
                        uint32_t* hits, uint8_t* sha1, uint8_t* o1, size_t cap, size_t* total) {
  ZPQ_TRY
  fragment_args(in, len, n, blocksize, nfrag, total);
  *total = 0;
  if (engine_device_count() <= 0) fail(ZPQ_E_UNSUPPORTED, "fragmenting on the device unavailable: no device");
  const FragLimits lim = fragment_limits(fragment, blocksize);
  std::vector<std::vector<Fragment>> fr;
  std::string note;
  if (engine_fragment(in, len, n, lim, fr, note) != 1) fail(ZPQ_E_UNSUPPORTED, "fragmenting on the device unavailable: " + note);
  return fragment_deliver(fr, n, nfrag, size, hits, sha1, o1, cap, total);
  ZPQ_CATCH
}

uint32_t zpq_last_fragment_rounds(void) { return engine_last_fragment_rounds(); }

uint32_t zpq_fragment_analyze(const uint8_t* o1, uint64_t sz, uint32_t hits, const uint8_t* o1prev, int* text1, int* exe1) {
  if (!o1 || !o1prev) return hits;
  return fragment_analyze(o1, sz, hits, o1prev, text1, exe1);
}

int zpq_sha1_batch_device(const uint8_t* const* in, const uint32_t* len, uint32_t n, uint8_t* out20n) {
  ZPQ_TRY
  if (n && (!in || !len || !out20n)) fail(ZPQ_E_ARG, "null argument");
  engine_sha1_host(in, len, n, out20n);
  return ZPQ_OK;
  ZPQ_CATCH
}

int zpq_last_api_timing(double out[8]) {
  if (!out) return ZPQ_E_ARG;
  const ApiTiming t = last_api_timing();
  out[0] = t.total_ms; out[1] = t.front_ms; out[2] = t.device_ms; out[3] = t.stitch_ms;
  out[4] = t.kernel_init_ms; out[5] = t.kernel_code_ms; out[6] = (double)t.blocks; out[7] = (double)t.sa_device_blocks;
  return ZPQ_OK;
}

uint32_t zpq_last_hash_parse_blocks(void) { return last_api_timing().hash_parse_blocks; }
uint32_t zpq_last_device_coded_blocks(void) { return last_api_timing().device_coded_blocks; }

size_t zpq_table(int which, void* out, size_t cap) {
  try {
    const Tables& t = tables();
    const void* src; size_t n;
    switch (which) {
      case 0: src = t.squash; n = sizeof(t.squash); break;
      case 1: src = t.stretch; n = sizeof(t.stretch); break;
      case 2: src = t.dt; n = sizeof(t.dt); break;
      case 3: src = t.dt2k; n = sizeof(t.dt2k); break;
      case 4: src = t.ns; n = sizeof(t.ns); break;
      case 5: src = t.icm_init; n = sizeof(t.icm_init); break;
      case 6: src = t.isse_init; n = sizeof(t.isse_init); break;
      case 7: src = t.sse_row; n = sizeof(t.sse_row); break;
      case 8: src = t.stretch_cb; n = sizeof(t.stretch_cb); break;
      case 9: src = t.stretch_top; n = sizeof(t.stretch_top); break;
      default: return 0;
    }
    if (n > cap) return 0;
    memcpy(out, src, n);
    return n;
  } catch (...) { return 0; }
}

}  // extern "C"
