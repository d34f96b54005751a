/* include/zpaq_amd.h -- the drop-in boundary: a thin C ABI over the MI355X engine.
 *
 * Plain C types, caller-owned buffers, integer status codes, no exceptions and
 * no torch types across this line.  Everything above it (the libzpaq-compatible
 * C++ classes in include/libzpaq.h, the Python mirror in zpaq_amd/) is host
 * plumbing; everything below it is HIP for gfx950.
 *
 * Each entry point names the reference interface it replaces (file:line into
 * zpaq 7.15's libzpaq.h / libzpaq.cpp).  The library is thread-safe: concurrent
 * callers are serialised on the device queue, mirroring how zpaq.cpp:1947 calls
 * compressBlock() from many threads.
 *
 * There is NO CPU fallback for the modelled path: if no gfx950 device/kernels
 * are available these functions return ZPQ_E_DEVICE, they never silently code
 * on the host.
 */
#ifndef ZPAQ_AMD_H
#define ZPAQ_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (per call and per block) ---- */
enum {
  ZPQ_OK = 0,
  ZPQ_E_NOMEM = 1,     /* "Out of memory" (libzpaq.h:925)                         */
  ZPQ_E_CORRUPT = 2,   /* "archive corrupted" (libzpaq.cpp:2108)                 */
  ZPQ_E_OVERFLOW = 3,  /* caller's output buffer too small                        */
  ZPQ_E_HEADER = 4,    /* bad COMP/HCOMP header (libzpaq.cpp:887-931, 1776-1846) */
  ZPQ_E_VM = 5,        /* "ZPAQL execution error" (libzpaq.cpp:1265)             */
  ZPQ_E_EOF = 6,       /* "unexpected end of file" (libzpaq.cpp:2120)            */
  ZPQ_E_DEVICE = 7,    /* no usable gfx950 device / HIP runtime error            */
  ZPQ_E_UNSUPPORTED = 8, /* valid ZPAQ feature outside this build's hot-path scope */
  ZPQ_E_ARG = 9
};

/* Thread-local text for the last failing call on this thread. */
const char* zpq_last_error(void);
const char* zpq_version(void);

/* ---- device ---- */
/* device >= 0: bind the engine to that HIP device (one process per GPU; without a call LOCAL_RANK picks it).
 * device == -1: drive EVERY visible GPU from this process (or the list in ZPAQ_AMD_DEVICES = "all" | "0,2,3"):
 * one engine per device, host-buffer batches (zpq_encode_batch, zpq_decode_batch, zpq_compress_blocks,
 * zpq_decompress, the libzpaq C++ classes) are sharded over them; the device-resident entry points keep using
 * the first one.  Idempotent.  Uploads the predictor's constant tables (squash/stretch/dt/
 * dt2k/state table; Predictor::init libzpaq.cpp:1731-1761) after verifying the
 * reference's two table checksums (1759-1760) on the host. */
int zpq_init(int device);
int zpq_device_count(void);
/* Engines zpq_init() configured: 1, or one per device named by zpq_init(-1) / ZPAQ_AMD_DEVICES (a device named twice gets two). */
int zpq_engine_count(void);
/* How a host-buffer batch of n blocks is split when the engine drives several GPUs (zpq_init(-1) or
 * ZPAQ_AMD_DEVICES=all|0,1,..): shard k of `parts` codes blocks [lo, hi) -- contiguous ranges, so archive order is
 * kept; one engine and one host thread per device, no collective (blocks are independent, libzpaq.h:57-59). */
void zpq_shard_range(uint64_t n, uint32_t parts, uint32_t k, uint64_t* lo, uint64_t* hi);
void zpq_shutdown(void);
/* Cap on device bytes the engine may hold for model state (default: 85% of
 * free HBM at init).  Batches needing more are run in several residency waves. */
int zpq_set_state_budget(uint64_t bytes);
/* Select the coding kernel: 0 = auto (best available for each plan: the pipelined encoder for compression, the
 * per-header specialised wavefront kernel for decompression), 1 = generic one-lane kernel, 2 = generic
 * wave-parallel kernel, 3 = per-header specialised wavefront kernel in both directions (one block per wavefront),
 * 4 = pipelined encoder (decompression as with 3), 5 = the decoder with two blocks per wavefront (compression as with 0),
 * 6 = the lockstep decoder (row / mixer wavefronts, the 8 blocks of a workgroup bit by bit together: what 0 picks for a
 * launch of more than 4 x CUs blocks whose chain it takes; compression as with 0).  3, 4, 5 and 6 fail with
 * ZPQ_E_UNSUPPORTED when the kernel cannot be built. */
int zpq_set_kernel(int which);

/* ---- model plan: a parsed block header + device arena layout ---- */
typedef struct zpq_plan zpq_plan;
/* header = hsize_lo hsize_hi hh hm ph pm n COMP.. 0 HCOMP.. 0 exactly as stored
 * in the archive.  Replaces ZPAQL::read (libzpaq.cpp:887) + the sizing half of
 * Predictor::init (1776-1846). */
int zpq_plan_create(const uint8_t* header, size_t hlen, zpq_plan** out);
void zpq_plan_destroy(zpq_plan*);
int zpq_plan_ncomp(const zpq_plan*);
/* ZPAQL::memory() (libzpaq.cpp:986-1006): what findBlock(&mem) reports. */
double zpq_plan_memory(const zpq_plan*);
/* Device bytes one in-flight block of this plan occupies. */
uint64_t zpq_plan_state_bytes(const zpq_plan*);
/* ALGORITHMIC model-state bytes moved per coded input byte,
 * excluding init and I/O: the roofline numerator. */
double zpq_plan_algo_bytes_per_byte(const zpq_plan*);

/* Per-header kernel specialisation (the GPU analogue of the reference's x86
 * JIT, libzpaq.cpp:3824-4583 / 3231-3811): HIP source generated for this
 * header, instantiating device/spec_kernel.h.  zpq_plan_spec_source returns the
 * text and its cache key (40 hex chars + NUL) so that a build step can
 * precompile it to <cache dir>/<key>.hsaco; at run time the engine loads that
 * file or falls back to hipRTC.  Needs no GPU. */
int zpq_plan_spec_source(const zpq_plan*, char* src, size_t cap, size_t* len, char key41[41]);
/* The same for the pipelined ENCODER of this header (device/pipe_kernel.h: one lane per block and component,
 * components connected by streams in HBM; used for compression whenever the chain supports it), and its
 * dataflow plan: out[0] bytes of stream buffer per group of blocks, [1] ring slots, [2] chunk bytes,
 * [3] units in the light kernel, [4] ICM maps, [5] ISSE maps, [6] MIX wavefronts per group, [7] blocks per HCOMP
 * workgroup, [8] highest dataflow level (a batch of L-byte blocks takes ceil(L / chunk) + out[8] steps),
 * [9] blocks per group (= threads per workgroup of every kernel but hcomp, which has 64), [10] ROW units,
 * [11] threads per workgroup of the mix kernel, [12] of the rows kernel, [13] of the light kernel.
 * The encoder has two shapes per chain: mode 0 "throughput" (a lane per block; batches that fill the GPU) and mode 1
 * "latency" (MIX / CM / MIX2 with a lane per bit position as well; the engine uses it for chains with at most 640 blocks
 * in the batch), mode 2 = mode 1 with 2048-byte steps (blocks of 128 KiB and more).  The plain calls give mode 0; the
 * _opts calls take the mode and, for tests, the chunk (bytes per step, 0 = the mode's own) and the group (blocks per
 * wavefront, 0 = 32). */
/* The decoder with two blocks per wavefront (device/spec_dual_kernel.h): chains of up to 32 components. */
int zpq_plan_spec_dual_source(const zpq_plan*, char* src, size_t cap, size_t* len, char key41[41]);
/* The lockstep decoder (device/spec_team_kernel.h): the 8 blocks of a workgroup advance bit by bit together, their ICM /
 * ISSE components on row wavefronts (16 lanes per block), everything else on mixer wavefronts (two blocks each).  Chains of
 * up to 32 components whose ISSEs are fed by the ICM / ISSE right before them. */
int zpq_plan_spec_team_source(const zpq_plan*, char* src, size_t cap, size_t* len, char key41[41]);
int zpq_plan_pipe_source(const zpq_plan*, char* src, size_t cap, size_t* len, char key41[41]);
int zpq_plan_pipe_layout(const zpq_plan*, uint64_t out[16]);
int zpq_plan_pipe_source_opts(const zpq_plan*, int mode, int chunk, int group, char* src, size_t cap, size_t* len, char key41[41]);
int zpq_plan_pipe_layout_opts(const zpq_plan*, int mode, int chunk, int group, uint64_t out[16]);
/* The same for a block's PCOMP post-processing program (device/pcomp_kernel.h: LZ77 / BWT / E8E9 inverses run one
 * lane per segment on the device when a batch has enough of them): code = the PCOMP bytes without their 2-byte
 * length, ph / pm = header bytes 4 and 5. */
int zpq_pcomp_source(const uint8_t* code, size_t codelen, int ph, int pm, char* src, size_t cap, size_t* len, char key41[41]);
/* Host post-processing (PostProcessor::write, libzpaq.cpp:2195-2241): 1 when this PCOMP program (bytes as for
 * zpq_pcomp_source) is one of those compressBlock's own methods generate, which the host runs as C++ translated at build time
 * (the counterpart of the reference's x86 JIT, libzpaq.cpp:3231-3811); 0 when it will be interpreted. */
int zpq_pcomp_is_translated(const uint8_t* code, size_t codelen, int ph, int pm);
/* Runs only the hipRTC compilation of that source (needs no GPU; nothing is loaded or cached):
 * returns the size of the gfx950 code object, or 0 with the compiler log in `log`. */
size_t zpq_plan_spec_jit(const zpq_plan*, char* log, size_t cap);
size_t zpq_plan_spec_dual_jit(const zpq_plan*, char* log, size_t cap);      /* the decoder with two blocks per wavefront */
size_t zpq_plan_spec_team_jit(const zpq_plan*, char* log, size_t cap);      /* the lockstep decoder */
/* Headers nobody prebuilt (level-5 chains whose periodic models depend on the data): compile the kernels of `n` plans
 * with hipRTC on up to `threads` host threads at once (0 = as many as the process may use, at most 16) -- the pipelined
 * encoder when decode == 0, the wavefront kernel otherwise -- into the code-object cache.  The engine does the same at
 * the start of every batch that brings more than one unseen header (at most ZPAQ_AMD_MAX_JIT = 64 per call); calling
 * it ahead of time (a caller that knows its methods) moves the cost out of the first batch.  Needs no GPU.
 * Returns the number of code objects compiled, or < 0. */
int zpq_precompile(const zpq_plan* const* plans, size_t n, int decode, int threads);
/* Introspection for tools and tests: the plan as the kernels see it (device/layout.h: PlanHeader,
 * CompDesc[n], Segment[nseg], HCOMP bytes).  The pointer stays valid until zpq_plan_destroy. */
const uint8_t* zpq_plan_blob(const zpq_plan*, size_t* len);
/* Which kernel will code this plan on the current device: 4 pipelined encoder (compression only), 3 specialised,
 * 2 generic wave, 1 generic one-lane.  note (optional) receives where the
 * specialised kernel came from ("cache:<key>" / "hiprtc") or why it is not used. */
int zpq_plan_kernel_kind(zpq_plan*, char* note, size_t cap);            /* compression */
int zpq_plan_kernel_kind2(zpq_plan*, int decode, char* note, size_t cap);
/* ... for a batch that holds nblocks blocks of this plan (the encoder's mode and the decoder's workgroup shape depend on it) */
int zpq_plan_kernel_kind3(zpq_plan*, int decode, uint32_t nblocks, char* note, size_t cap);
/* ... whose longest block has block_bytes bytes (latency shape: 2048-byte steps for blocks of 128 KiB and more) */
int zpq_plan_kernel_kind4(zpq_plan*, int decode, uint32_t nblocks, uint32_t block_bytes, char* note, size_t cap);
/* The encoder variant (0 throughput shape, 1 latency shape, 2 latency shape with 2048-byte steps, 3 latency shape with a
 * wavefront per SIMD) the launch policy (device/launch_policy.hpp) gives every chain of a batch: chain i is blocks[i] blocks of
 * plans[i], the longest of longest[i] bytes, on a device of `cus` compute units in `xcds` compute dies (XCDs);
 * persist_expected = the call waits for its results (zpq_*_device with timed = 0 does not).  The knobs of the environment
 * (ZPAQ_AMD_PIPE_PERSIST / _MODE / _WIDE) count as they do for a batch.  Touches no device. */
int zpq_encoder_variants(const zpq_plan* const* plans, const uint32_t* blocks, const uint32_t* longest, uint32_t nchains,
                         int cus, int xcds, int persist_expected, int32_t* variants);
/* Directories used by the specialisation cache / hipRTC include path. */
const char* zpq_spec_cache_dir(void);
const char* zpq_spec_include_dir(void);

/* ---- the hot path: batches of independent blocks ---- */
/* Encoder::compress over in[b][0..in_len[b]) then EOS, for every block
 * (libzpaq.cpp:2419-2447 driving Predictor::predict/update 1854-2066 and
 * ZPAQL::run 1027).  `in[b]` is what the Compressor feeds the Encoder: PP header
 * byte(s) then data.  out[b] receives the coded bytes including the 4 EOS
 * flush bytes (not the 00 00 00 00 terminator).  status[b] is per block.
 * Host pointers; the call copies in, runs, copies out. */
int zpq_encode_batch(const zpq_plan* const* plans, const uint8_t* const* in,
                     const uint32_t* in_len, uint32_t nblocks,
                     uint8_t* const* out, const uint32_t* out_cap,
                     uint32_t* out_len, int32_t* status);

/* Decoder::decompress until EOS for every block (libzpaq.cpp:2127-2155).
 * in[b] = coded bytes starting at the first coded byte and including at least
 * the 4-zero terminator.  out[b] gets the decoded bytes (PP header included);
 * consumed[b] = coded bytes read (terminator included).  max_out[b] bounds the
 * decode ("decode first k bytes", Decompresser::decompress(n) 2315): decoding
 * stops early with status ZPQ_OK and consumed = 0 when max_out is reached
 * before EOS. */
int zpq_decode_batch(const zpq_plan* const* plans, const uint8_t* const* in,
                     const uint32_t* in_len, uint32_t nblocks,
                     uint8_t* const* out, const uint32_t* max_out,
                     uint32_t* out_len, uint32_t* consumed, int32_t* status);

/* Device-resident variants (inputs already in HBM; used by bench.py and by
 * callers that keep data on the GPU).  d_in/d_out are DEVICE pointers; block b
 * reads d_in + in_off[b] and writes d_out + out_off[b] (in_off/in_len/out_off/
 * out_cap are HOST arrays).  Per-block results land in the DEVICE array d_res.
 * `stream` is a hipStream_t (NULL = the engine's own stream).  One plan for the
 * whole batch, which must fit the state budget.  Of block b's output region
 * [out_off[b], out_off[b] + out_cap[b]) the first out_len bytes are the result;
 * what the rest holds afterwards is undefined (the coder of small batches stores
 * four bytes per coded bit and lets the next store overwrite what was not yet
 * final), nothing outside the region is written.  The call enqueues
 * init_arena + the coding kernel on `stream`; with timed!=0 it also brackets
 * them with hipEvents on that stream, waits, and makes the durations available
 * through zpq_last_timing(). */
typedef struct zpq_block_result {
  uint32_t out_len;    /* bytes produced                                   */
  uint32_t consumed;   /* decode: coded bytes read incl. terminator, 0 if stopped at max_out */
  int32_t status;      /* ZPQ_* per block                                  */
  uint32_t steps;      /* predict/update steps executed (coded bits)       */
} zpq_block_result;

int zpq_encode_device(const zpq_plan* plan, const void* d_in, const uint64_t* in_off,
                      const uint32_t* in_len, uint32_t nblocks, void* d_out,
                      const uint64_t* out_off, const uint32_t* out_cap,
                      zpq_block_result* d_res, void* stream, int timed);
int zpq_decode_device(const zpq_plan* plan, const void* d_in, const uint64_t* in_off,
                      const uint32_t* in_len, uint32_t nblocks, void* d_out,
                      const uint64_t* out_off, const uint32_t* max_out,
                      zpq_block_result* d_res, void* stream, int timed);
/* Same, with one plan PER BLOCK (plans[b]): blocks are grouped by plan internally and the groups
 * run concurrently on side streams; results keep the caller's block order.  decode = 0 / 1. */
int zpq_code_device_multi(int decode, const zpq_plan* const* plans, const void* d_in,
                          const uint64_t* in_off, const uint32_t* in_len, uint32_t nblocks,
                          void* d_out, const uint64_t* out_off, const uint32_t* cap,
                          zpq_block_result* d_res, void* stream, int timed);
/* Durations (ms, hipEvent) of the last timed call on this process: Predictor
 * init kernel and coding kernel(s); blocks = blocks they covered. */
int zpq_last_timing(float* init_ms, float* code_ms, uint32_t* blocks);
/* 1 when the pipelined encoder of the last timed call ran as persistent launches (one launch per chain for the whole
 * sequence, device/pipe_persist.h), 0 when it ran step by step (or the call had no pipelined group). */
int zpq_last_persistent(void);
/* When a persistent launch of the last timed call was given up (its workgroups did not become resident together -- something
 * else held compute units -- or a unit's watchdog fired) and the step kernels coded the batch instead: milliseconds from the
 * launch until the engine knew; 0 when none was given up.  The arrival handshake bounds it to ~2 x 20 ms
 * (ZPAQ_AMD_PERSIST_ARRIVE_MS) and leaves the model state untouched. */
double zpq_last_persist_abort_ms(void);
/* SHA-1 (libzpaq::SHA1, libzpaq.cpp:106-177) of n buffers ON THE DEVICE, one lane per buffer, 20 bytes each into
 * out20n.  zpq_compress_blocks uses the same kernel for blocks that reach the device unchanged (methods without
 * pre-processing): the digest for the segment trailer is computed beside the coder instead of on a host thread. */
int zpq_sha1_batch_device(const uint8_t* const* in, const uint32_t* len, uint32_t n, uint8_t* out20n);
/* Wall-clock phases (ms) of this process's last zpq_compress_blocks call -- the end-to-end path through the
 * drop-in API: out[0] total, [1] host front half (SHA-1, method expansion, header assembly), [2] device call
 * (staging + H2D + kernels + D2H), [3] archive stitching, [4] / [5] the Predictor-init and coding kernels inside
 * [2] (hipEvents), [6] blocks. */
int zpq_last_api_timing(double out[8]);
/* Blocks of this process's last zpq_compress_blocks call whose LZ77 parse through LZBuffer's hash table (method 1, method 2
 * below type 64, x / s methods with args[5] - args[0] < 21) ran on the device (device/lz77_hash_kernel.h); 0 when the host
 * parsed them (a small batch, ZPAQ_AMD_DEVICE_PARSE=0, parameters outside the device's range, no device). */
uint32_t zpq_last_hash_parse_blocks(void);
/* Blocks of this process's last zpq_compress_blocks call whose LZ77 stream (LZBuffer's codes, libzpaq.cpp:6759-6883) was written
 * on the device from the list of matches the device's parse left there (device/lz77_codes_kernel.h): the finished stream came
 * back over PCIe instead of 16 bytes per match, and no host core walked the block again.  0 when the host wrote the codes: the
 * host parsed (see above), ZPAQ_AMD_DEVICE_CODES=0, or a batch for which it does not pay.
 *   ZPAQ_AMD_DEVICE_CODES=0|1: 0 keeps the download of the list and the host's coder (host/preproc.cpp lz77_serialize), 1 writes
 *   every such batch's codes on the device.  Unset, the engine decides per batch once the sizes are known: on the device when
 *   the streams are smaller than the lists (16 bytes per match) and not below 1 % of the input -- an incompressible batch has no
 *   matches, its list is empty and its stream is the input, so it stays with the host (measured: DESIGN 4.5.2).
 *   ZPAQ_AMD_DEVICE_PARSE=0 implies 0: there is no list on the device then.  The archives are the same either way. */
uint32_t zpq_last_device_coded_blocks(void);
/* Runs a tiny kernel exercising the cross-lane idioms (DPP reduction, readlane,
 * bpermute); out8[0..5] must equal {2016, 21344, 123, 2016, 133, 13671}. */
int zpq_selftest(int32_t out8[8]);

/* ---- block-level drop-ins (host side + hot path) ---- */
/* Batched libzpaq::compressBlock (libzpaq.h:1505, libzpaq.cpp:7543): each
 * in[b] becomes one ZPAQ block with one segment, bit-identical to the
 * reference's output for the same (method, filename, comment, dosha1).
 * in[b] may be modified in place exactly where the reference would (E8E9).
 * out_len[b] always receives the needed size; ZPQ_E_OVERFLOW if cap too small. */
int zpq_compress_blocks(const char* method, uint8_t* const* in, const uint32_t* in_len,
                        uint32_t nblocks, const char* const* filename,
                        const char* const* comment, int dosha1,
                        uint8_t* const* out, const uint64_t* out_cap, uint64_t* out_len);

/* libzpaq::decompress (libzpaq.h:1268, libzpaq.cpp:2378) over a whole archive
 * (any number of blocks/segments): all blocks are located on the host, decoded
 * on the device as one batch, and concatenated in order.  Verifies segment
 * SHA-1 trailers when present (status ZPQ_E_CORRUPT on mismatch). */
int zpq_decompress(const uint8_t* archive, uint64_t n, uint8_t* out, uint64_t cap,
                   uint64_t* out_len);
/* Work bound for archives from untrusted sources: the ZPAQL steps ONE call of a block's own (non-standard) PCOMP
 * post-processor may take before the block is rejected with ZPQ_E_VM.  The reference (PostProcessor / ZPAQL::run,
 * libzpaq.cpp:1310-1330, 2236-2330) has no bound at all and a damaged program loops for good; the default here is 2^34
 * (about a minute), which no useful program comes near.  0 restores the default.  Process-wide. */
void zpq_set_pcomp_step_limit(uint64_t steps);

/* ---- host-side pieces of the boundary, exposed for reuse and for tests ---- */
/* SHA1 (libzpaq.h:934-954). */
void zpq_sha1(const uint8_t* in, uint64_t n, uint8_t out20[20]);
/* tests: 1 = hash with the portable compression function instead of the x86 SHA extensions (0 = back to automatic) */
void zpq_sha1_force_portable(int yes);
/* Suffix arrays (the sort inside the byte-aligned LZ77 and BWT pre-processors of methods 2-4; reference: divsufsort,
 * libzpaq.cpp:4658-6434, called from LZBuffer 6463-6883 and compressBlock 7709-7716) of n host buffers in ONE device
 * call: out[i] receives len[i] positions, the end of the string ordered before every byte.  zpq_compress_blocks uses
 * this by itself for batches with 4 or more such blocks; ZPQ_E_UNSUPPORTED when the device declines (a buffer of 16 MiB
 * or more, more than 65 535 buffers, not enough memory) -- the library then sorts on the host. */
int zpq_suffix_arrays_device(const uint8_t* const* in, const uint32_t* len, uint32_t n, uint32_t* const* out);
/* ONE buffer of any length below 2^31 bytes through the wide sorter (device/sa_wide_kernel.h: no block id in the key, two rank
 * fields of up to 31 bits, 32 bytes of device memory per byte): out receives n positions, the end of the string ordered before
 * every byte.  ZPQ_E_UNSUPPORTED with a note in zpq_last_error when there is no device, the length is outside the range or the
 * block does not fit the device budget; out is untouched then.  zpq_compress_blocks sends its sorting blocks of 2^24 bytes and
 * more this way (ZPAQ_AMD_DEVICE_SORT_WIDE unset: from 16 MiB + 4096 bytes, the smallest size measured; 1: all of them; 0: never);
 * ZPAQ_AMD_SORT_WIDE_FROM=<bytes>, read per call, moves that split (tests).  zpq_last_wide_sort_blocks: the blocks of this
 * process's last zpq_compress_blocks call that the wide sorter sorted; zpq_last_wide_sort_rounds: the doubling rounds of this
 * process's last wide sort. */
int zpq_suffix_array_device_wide(const uint8_t* in, uint32_t n, uint32_t* out);
uint32_t zpq_last_wide_sort_blocks(void);
uint32_t zpq_last_wide_sort_rounds(void);
/* zpq_preprocess_block for one buffer with the sort by the wide sorter, for any method whose pre-processor sorts suffixes and
 * any n below 2^31: a BWT method's last column is made on the device; an LZ77 method is parsed by the host with the device's
 * array, or -- ZPAQ_AMD_DEVICE_PARSE_WIDE=1; unset: where the measured rule says so, DESIGN 4.5.9 -- on the device in pieces
 * (device/lz77_wide_kernel.h), its codes written there as well as ZPAQ_AMD_DEVICE_CODES says.  Byte for byte
 * zpq_preprocess_block's stream whichever path makes it; *len is always reported and nothing is written when cap is short
 * (ZPQ_E_OVERFLOW).  ZPQ_E_UNSUPPORTED for a method that does not sort suffixes, without a device, or when the device
 * declines; `data` is then as it came (an E8E9 method's filter is taken back on every failure). */
int zpq_preprocess_block_device_wide(const char* xmethod, uint8_t* data, uint32_t n, uint8_t* out, size_t cap, size_t* len);
/* The LZ77 parse of ONE buffer of any length below 2^31 on the device: E8E9 in place as the method says, the wide sort, then the
 * search (a lane per position), the walk of pieces of 64 KiB from provisional starts (a wavefront each), the stitch that adopts
 * a piece's list where the true walk meets it in an identical state, and the gather (device/lz77_wide_kernel.h).
 * The list in zpq_lz77_tokens_host's layout, token for token the host's; *count is always reported and nothing is written when
 * cap is short (ZPQ_E_OVERFLOW).  ZPQ_E_UNSUPPORTED with a note in zpq_last_error for a method whose LZ77 does not search a suffix
 * array (or that is no LZ77), without a device, for input outside the range (min_match >= 1, lookahead <= 255, 1 <= checkbits
 * <= 31, offset bits <= 7), or when the sort and the parse do not fit the device budget; `data` is as it came on every failure.
 * ZPAQ_AMD_LZ_WIDE_PIECE=<bytes>, read per call, overrides the piece size (clamped to [64, 2^30], rounded up to a multiple of
 * 64: tests).
 * zpq_compress_blocks parses a wide LZ77 block this way with ZPAQ_AMD_DEVICE_PARSE_WIDE=1 (0: never; unset: where the measured
 * rule says so, never below 2^24 bytes; ZPAQ_AMD_DEVICE_PARSE=0 wins: sort only); archives are identical whichever path parses
 * and codes.  zpq_last_wide_parse_blocks: the blocks of this process's last zpq_compress_blocks call that were parsed there.
 * zpq_last_wide_parse_pieces, of this process's last wide parse: pieces, pieces adopted whole, pieces re-joined after a re-walk,
 * pieces that contributed only re-walked tokens or nothing (the four add up).
 * zpq_wide_stage_bytes: what a wide call for a block of n bytes holds on the device, as its budget check sums it -- out2[0] the
 * sort alone, out2[1] the sort with the parse and the coder's arrays (equal for a BWT method).  A block whose second sum exceeds
 * the budget but whose first does not is sorted there and parsed by the host.  Needs no device. */
int zpq_lz77_parse_device_wide(const char* xmethod, uint8_t* data, uint32_t n, uint32_t* tokens4, size_t cap, size_t* count);
uint32_t zpq_last_wide_parse_blocks(void);
void zpq_last_wide_parse_pieces(uint32_t out4[4]);
int zpq_wide_stage_bytes(const char* xmethod, uint32_t n, uint64_t out2[2]);
int zpq_suffix_array_host(const uint8_t* in, uint32_t n, uint32_t* out);      /* the host's sorter (SA-IS), one buffer */
/* compressBlock's level->method expansion (libzpaq.cpp:7579-7691), including
 * level-5 period detection on the data.  Writes a NUL-terminated "x..." /
 * "0..." string. */
int zpq_expand_method(const char* method, const uint8_t* data, uint32_t n, char* out, size_t cap);
/* makeConfig + Compiler (libzpaq.cpp:6887, 2698): "x..." method -> block header
 * bytes as stored (hcomp) and the PCOMP bytes the Compressor codes through the
 * model (len16 + code, empty if none); args9 receives $1..$9. */
int zpq_method_to_header(const char* xmethod, int* args9, uint8_t* hcomp, size_t hcap,
                         size_t* hlen, uint8_t* pcomp, size_t pcap, size_t* plen);
/* The stored block header of built-in model `level` (1 min.cfg, 2 mid.cfg, 3 max.cfg): what
 * Compressor::startBlock(int level) writes (libzpaq.cpp:2793-2839).  Feed it to zpq_plan_create to code blocks
 * with the legacy models through the batch entry points (the coder's input is then a 0 byte + the data:
 * Compressor::postProcess(NULL), libzpaq.cpp:2853-2870). */
int zpq_builtin_model_header(int level, uint8_t* hcomp, size_t hcap, size_t* hlen);
/* The pre-processing half of compressBlock for an explicit "x.." method (libzpaq.cpp:7709-7716; LZ77 / BWT /
 * E8E9, host/preproc.cpp): writes the stream the coder will see (the input itself when the method does not
 * transform it).  E8E9 methods rewrite `data` in place, as the reference rewrites its input buffer. */
int zpq_preprocess_block(const char* xmethod, uint8_t* data, uint32_t n, uint8_t* out, size_t cap, size_t* len);
/* The same with the suffix array of the block supplied (zpq_suffix_arrays_device / zpq_suffix_array_host): what
 * zpq_compress_blocks does for a batch.  For a method with E8E9 (x.,5 / x.,6 / x.,7) the caller filters first with
 * zpq_e8e9 -- the suffixes sorted are those of the filtered bytes -- and this call then does not filter again. */
int zpq_preprocess_block_sa(const char* xmethod, uint8_t* data, uint32_t n, const uint32_t* sa, uint8_t* out, size_t cap, size_t* len);
/* The pre-processors behind the sort for n buffers in one device call: the suffix sort, the LZ77 parse (LZBuffer::fill with a
   suffix array, libzpaq.cpp:6693-6757) and the BWT's last column run on the GPU (device/lz77_kernel.h), the parse comes back
   as a list of matches (4 x uint32: position of the search, offset, length, literals in front) and the host writes LZBuffer's
   codes from it (6759-6883).  Methods whose LZ77 searches the hash table instead (args[5] - args[0] < 21; 6702-6782) are
   parsed by device/lz77_hash_kernel.h the same way, without a sort of suffixes.  zpq_preprocess_blocks_device returns what
   zpq_preprocess_block does, buffer by buffer; zpq_lz77_tokens_host is the host's list (either search), zpq_lz77_serialize
   the coder. */
int zpq_preprocess_blocks_device(const char* xmethod, uint8_t* const* data, const uint32_t* len, uint32_t n, uint8_t* const* out, const size_t* cap,
                                 size_t* outlen);
int zpq_lz77_tokens_host(const char* xmethod, uint8_t* data, uint32_t n, uint32_t* tokens4, size_t cap, size_t* count);
int zpq_lz77_serialize(const char* xmethod, const uint8_t* data, uint32_t n, const uint32_t* tokens4, size_t ntok, uint8_t* out, size_t cap, size_t* len);
/* zpq_lz77_serialize for a batch, with the codes written on the device (device/lz77_codes_kernel.h): token lists tokens4[b]
 * (ntok[b] matches of 4 x uint32) over the already filtered blocks data[b] of len[b] bytes; out[b] receives block b's stream,
 * outlen[b] its size.  The contract of the host's entry, list by list: every size is reported also when some buffer is too
 * small (ZPQ_E_OVERFLOW; nothing is written then), a list the host's coder refuses -- matches out of order, offset 0 or
 * beyond the position, length 0, a span past the end of the block -- is refused with ZPQ_E_DEVICE and nothing is emitted.
 * ZPQ_E_UNSUPPORTED with a note in zpq_last_error when there is no device or the batch lies outside the device's range: blocks
 * below 2^24 bytes, at most 65 535 blocks, 2 GiB per batch, an LZ77 method of level 1 or 2. */
int zpq_lz77_serialize_device(const char* xmethod, const uint8_t* const* data, const uint32_t* len, const uint32_t* const* tokens4, const size_t* ntok,
                              uint32_t nblocks, uint8_t* const* out, const size_t* cap, size_t* outlen);
/* The method's own PCOMP program over one stream on the HOST (host/postproc.cpp): the inverse of zpq_preprocess_block, what
 * zpq_decompress does with a segment behind the model.  A method without a program passes the stream through.  outlen always
 * receives the size; ZPQ_E_OVERFLOW when cap is too small (nothing is written), ZPQ_E_VM when the program stops with an error. */
int zpq_postprocess_block(const char* xmethod, const uint8_t* stream, uint32_t len, uint8_t* out, size_t cap, size_t* outlen);
/* The same for a batch of LZ77 streams (level 1 / 2, no E8E9) on the device (device/lz77_decode_kernel.h, a wavefront per
 * stream).  status[b]: 0 decoded -- out[b] holds, byte for byte, what zpq_postprocess_block makes of stream b, outlen[b] its
 * size; 1 declined -- out[b] is untouched and the caller runs the program on the host: a match that reaches in front of the
 * output, a length of 0, an output beyond the program's 2^(args[0] + 20) bytes, a field beyond the program's registers.  The
 * device never gives a verdict on a damaged stream, and it declines no stream this library's coder writes.  How a stream ends
 * is the program's: an unfinished code is dropped, an unfinished run of literals keeps the bytes that arrived.
 * Every size is reported also when a buffer is too small (ZPQ_E_OVERFLOW, nothing written); ZPQ_E_UNSUPPORTED with a note in
 * zpq_last_error without a device, for another kind of method, or outside the range (65 535 streams and 2 GiB of output per
 * batch, 16 bytes of workspace per stream byte within the device budget). */
int zpq_lz77_decode_device(const char* xmethod, const uint8_t* const* stream, const uint32_t* len, uint32_t n,
                           uint8_t* const* out, const size_t* cap, size_t* outlen, int32_t* status);
/* Segments of this process's last zpq_decompress call that device/lz77_decode_kernel.h decoded.  A segment qualifies when its
 * block has one segment and carries, byte for byte, one of the LZ77 programs without E8E9 that compressBlock's methods generate
 * (methods 1 and 2, the LZ77 branches of 3 and 4, x.,1.. / x.,2..); E8E9 variants, BWT, custom programs and blocks of several
 * segments never do.  ZPAQ_AMD_DEVICE_UNLZ=0|1 forces the route off or on for qualifying segments; unset it is taken by
 * groups of 256 segments and more, the smallest batch at which it was faster than both other routes.  Any set
 * value of ZPAQ_AMD_PCOMP keeps its meaning and the counter at 0.  The bytes are the same either way. */
uint32_t zpq_last_device_unlz_segments(void);
/* The same batch through the decoder for LONG streams (device/lz77_decode_wide_kernel.h): a stream is parsed in
 * pieces of 16 KiB from provisional starts, a wavefront each; one wavefront per stream stitches the pieces' lists along the true
 * walk (the code stream re-synchronises by itself); the checks that need the absolute output position follow, a lane per token;
 * and the copy is pointer jumping over a word per output byte, no lane waiting for another.  The argument list, the status
 * meanings and the contract per stream are zpq_lz77_decode_device's; a stream of any length is taken, a short one too.  Range:
 * 65 535 streams, outputs below 2^31 bytes per stream and per batch; 36 bytes per stream byte (rounded up to whole pieces), 4
 * bytes per output byte, the streams and the outputs within the device budget.  ZPQ_E_OVERFLOW with every size reported and
 * nothing written when a decoded block does not fit its buffer; ZPQ_E_UNSUPPORTED with a note without a device, for another
 * kind of method, or outside the range.  ZPAQ_AMD_UNLZ_WIDE_PIECE=<bytes>, read per call, overrides the piece size (clamped to
 * [64, 2^20], rounded up to a multiple of 64: tests). */
int zpq_lz77_decode_device_wide(const char* xmethod, const uint8_t* const* stream, const uint32_t* len, uint32_t n,
                                uint8_t* const* out, const size_t* cap, size_t* outlen, int32_t* status);
/* Segments of this process's last zpq_decompress call that went that way.  Inside a group that qualifies for
 * zpq_last_device_unlz_segments' route, the segments whose stream has at least ZPAQ_AMD_UNLZ_WIDE_FROM bytes (default 1 MiB; read
 * per call: tests) are candidates; ZPAQ_AMD_DEVICE_UNLZ_WIDE=0|1 forces the route off or on for them.  Unset it is off: it is
 * taken only from a measured stream size at which it beat both other routes on every kind of data, and the measurement is not
 * complete yet (DESIGN 4.5.10 has the table of what was timed).  What it declines, and the rest of the group, goes on exactly as without it, ZPAQ_AMD_DEVICE_UNLZ included.
 * Any set value of ZPAQ_AMD_PCOMP keeps its meaning and the counter at 0; E8E9 groups never qualify.  The bytes are the same
 * either way. */
uint32_t zpq_last_device_unlz_wide_segments(void);
/* Of this process's last call of that decoder (zpq_lz77_decode_device_wide, or the route of zpq_decompress): pieces; pieces whose
 * list was adopted in the state the true walk entered them in; pieces met after a serial stretch; pieces walked serially to their
 * end (the rest: a code leapt over them) -- and the jump rounds of its longest copy. */
void zpq_last_unlz_wide_pieces(uint32_t out4[4]);
uint32_t zpq_last_unlz_wide_rounds(void);
/* The same for a batch of BWT streams (level 3 without E8E9, args[0] <= 4: x0,3 .. x4,3) on the device
 * (device/bwt_decode_kernel.h: a stable counting sort per tile, then the list ranked from every 256th node at once).  A stream
 * is S[0 .. n] and idx in 4 bytes, low byte first.  status[b]: 0 decoded -- out[b] holds, byte for byte, what
 * zpq_postprocess_block makes of stream b, outlen[b] its size (ff 00 00 00 00, the empty block, decodes to nothing); 1 declined
 * -- out[b] is untouched, outlen[b] is 0 and the caller runs the program on the host: a stream shorter than 5 bytes or outside
 * the rule 1 <= idx <= n and S[idx] == 255, n >= 2^24, n + 257 > 2^(args[0] + 20) (the program's counters would not fit), a
 * list whose path from idx has not exactly n nodes.  The device never gives a verdict on a damaged stream, and it declines no
 * stream this library's BWT writes.  Sizes are known before anything runs (n = len - 5): when an admitted stream does not fit
 * its buffer every size is reported and nothing is launched (ZPQ_E_OVERFLOW).  ZPQ_E_UNSUPPORTED with a note in zpq_last_error
 * without a device, for another kind of method, or outside the range (65 535 streams and 2 GiB of output per batch; 4 bytes of
 * workspace per stream byte, the tile histograms, the splitter tables and the outputs within the device budget). */
int zpq_bwt_decode_device(const char* xmethod, const uint8_t* const* stream, const uint32_t* len, uint32_t n,
                          uint8_t* const* out, const size_t* cap, size_t* outlen, int32_t* status);
/* The same for the program of a BWT method at args[0] 5 .. 11 -- xN,3 and, behind the inverse E8E9 filter, xN,7 for N in 5 .. 11,
 * the blocks of 16 MiB and more that the small decoder's 24-bit list word cannot hold (device/bwt_decode_wide_kernel.h, DESIGN
 * 4.5.8: 8 bytes per node, the splitter list ranked over second-level splitters).  The contract is zpq_bwt_decode_device's, per
 * stream: status 0 -- out[b] holds, byte for byte, what zpq_postprocess_block makes of stream b with that method; 1 declined,
 * out[b] untouched -- a stream shorter than 5 bytes or outside the rule, n + 257 > 2^(args[0] + 20), a path that has not n nodes,
 * for xN,7 a block the filter gave up, and a stream whose workspace does not fit the device budget alone.  A stream of any
 * admitted length is taken, a small one too.  A batch whose outputs exceed 2 GiB or whose workspace (8 bytes per stream byte, 1
 * KiB per tile, the two splitter tables, the streams and the outputs) exceeds the budget is cut into consecutive sub-batches.
 * ZPQ_E_OVERFLOW with every size reported and nothing launched when an admitted stream does not fit its buffer;
 * ZPQ_E_UNSUPPORTED with a note without a device, for another method (args[0] <= 4 among them: zpq_bwt_decode_device /
 * zpq_e8e9_decode_device), or when nothing of the batch fits the budget. */
int zpq_bwt_decode_device_wide(const char* xmethod, const uint8_t* const* stream, const uint32_t* len, uint32_t n,
                               uint8_t* const* out, const size_t* cap, size_t* outlen, int32_t* status);
/* Segments of this process's last zpq_decompress call that device/bwt_decode_kernel.h or, for the program at args[0] 5 .. 11,
 * device/bwt_decode_wide_kernel.h decoded.  A segment qualifies when its block has one segment and carries, byte for byte, the
 * BWT program without E8E9 that compressBlock's methods generate (the BWT branches of methods 3 and 4, x.,3..) with ph = pm =
 * args[0] + 20; E8E9 variants (zpq_last_device_une8_segments counts those), custom programs and blocks of several segments
 * never do.  ZPAQ_AMD_DEVICE_UNBWT=0|1 forces the route off or on for qualifying segments.  Unset, at args[0] <= 4 it is off:
 * it is taken only from a measured group size of 64 segments or more at which it beat both other routes, and no measurement
 * exists yet.  Unset, at args[0] 5 .. 11 it is on for a group of 2^24 + 4 097 stream bytes or more, the smallest
 * size measured (bwt_unbwt_wide_pays), and off below.  Any set value of ZPAQ_AMD_PCOMP keeps its meaning and the counter at 0.
 * The bytes are the same either way. */
uint32_t zpq_last_device_unbwt_segments(void);
/* The same for a batch of streams of an E8E9 method: args[1] = 4 (the filter alone: the stream is the filtered block), 5 / 6 (in
 * front of LZ77 level 1 / 2) or 7 (in front of the BWT, at args[0] <= 4 only).  The stream goes through the stage's decoder as
 * in zpq_lz77_decode_device / zpq_bwt_decode_device, with the method's own parameters, and the inverse filter runs over the
 * result while it is on the device (device/e8e9_kernel.h: the scan is serial only along chains of candidates, a lane walks each
 * from its first e8 / e9).  status[b]: 0 decoded -- out[b] holds, byte for byte, what zpq_postprocess_block makes of stream b,
 * outlen[b] its size; 1 declined -- out[b] is untouched, outlen[b] is 0 and the caller runs the program on the host: whatever
 * the stage in front declines (an output beyond 2^(args[0] + 20) bytes among it: the programs filter M, which wraps there), or
 * a chain that one lane did not finish in 2^20 serial steps.  The device never gives a verdict on a damaged stream.  When a
 * decoded block does not fit its buffer every size is reported and nothing is written (ZPQ_E_OVERFLOW).  ZPQ_E_UNSUPPORTED with
 * a note in zpq_last_error without a device, for another kind of method, or outside the range (65 535 streams and 2 GiB of
 * output per batch; the stage's workspace, the outputs and 4 bytes per e8 / e9 candidate and chain within the device budget). */
int zpq_e8e9_decode_device(const char* xmethod, const uint8_t* const* stream, const uint32_t* len, uint32_t n,
                           uint8_t* const* out, const size_t* cap, size_t* outlen, int32_t* status);
/* Segments of this process's last zpq_decompress call that went that way.  A segment qualifies when its block has one segment
 * and carries, byte for byte, one of the E8E9 programs compressBlock's methods generate: the filter alone (x.,4..), in front of
 * LZ77 (x.,5.., x.,6..) or in front of the BWT (x.,7..; at args[0] 5 .. 11 the stage in front is the wide BWT decoder of
 * zpq_bwt_decode_device_wide, and with the knob unset the route is off: no such group has been timed); custom programs and blocks of
 * several segments never do.  ZPAQ_AMD_DEVICE_UNE8=0|1 forces the route off or on for qualifying segments; unset it is off: it
 * is taken only from a measured group size of 64 segments or more at which it beat both other routes, and no measurement
 * exists yet.  Any set value of ZPAQ_AMD_PCOMP keeps its meaning and the counter at 0.  ZPAQ_AMD_DEVICE_UNLZ and
 * ZPAQ_AMD_DEVICE_UNBWT never touch these segments.  The bytes are the same either way. */
uint32_t zpq_last_device_une8_segments(void);
/* Streams of the E8E9 forms of the LZ77 methods -- args[1] = 5 or 6 at any args[0] 0 .. 11 -- through the decoder for LONG
 * streams (zpq_lz77_decode_device_wide: pieces, stitch, pointer jumping) and then the inverse filter, both on the device (DESIGN
 * 4.5.10): the copy's bytes are emitted into rooms placed for device/e8e9_kernel.h, each on a multiple of 16 bytes, and filtered
 * there before they go down.  The argument list and the statuses are zpq_e8e9_decode_device's and so is the contract per stream:
 * status 0 -- out[b] holds, byte for byte, what zpq_postprocess_block makes of stream b; 1 declined, out[b] untouched -- whatever
 * the wide LZ77 decoder declines, an output beyond 2^(args[0] + 20) bytes, or a chain a lane gave up.  A stream of any length
 * is taken.  Range and sub-batches as for zpq_lz77_decode_device_wide, with the rooms' padding, 8 bytes per 4 KiB of output and 4
 * bytes per e8 / e9 candidate and chain besides; the 2 GiB per batch are of the rooms.  ZPQ_E_OVERFLOW with every size reported
 * and nothing written when a decoded block does not fit its buffer; ZPQ_E_UNSUPPORTED with a note without a device, for another
 * kind of method, or outside the range.  zpq_last_unlz_wide_pieces and zpq_last_unlz_wide_rounds report this decoder's last call
 * as they do for zpq_lz77_decode_device_wide; ZPAQ_AMD_UNLZ_WIDE_PIECE sets the piece here too. */
int zpq_e8e9_decode_device_wide(const char* xmethod, const uint8_t* const* stream, const uint32_t* len, uint32_t n,
                                uint8_t* const* out, const size_t* cap, size_t* outlen, int32_t* status);
/* Segments of this process's last zpq_decompress call that went that way.  Inside a group that qualifies for
 * zpq_last_device_une8_segments' route with an x.,5 or x.,6 program, the segments whose stream has at least
 * ZPAQ_AMD_UNLZ_WIDE_FROM bytes (default 1 MiB; read per call) are candidates.  The route runs only when ZPAQ_AMD_DEVICE_UNE8 and
 * ZPAQ_AMD_DEVICE_UNLZ_WIDE are both 1; either at 0, or any set value of ZPAQ_AMD_PCOMP, keeps it off, and with one or both unset
 * it is off as well (e8_unlz_wide_pays; DESIGN 4.5.10 has the table and the rule).  What it decodes is counted here and in
 * neither zpq_last_device_une8_segments nor zpq_last_device_unlz_wide_segments; what it declines, and the rest of the group, goes
 * on exactly as without it, ZPAQ_AMD_DEVICE_UNE8's own route included.  The bytes are the same either way. */
uint32_t zpq_last_device_une8_wide_segments(void);
/* The forward E8E9 filter (e8e9, libzpaq.cpp:6450-6459) of n buffers on the device, in place: the stage on its own.  The scan
 * runs from the end of a buffer down and looks byte-serial; it is serial only along chains of e8 / e9 opcodes less than four
 * bytes apart, and a lane walks each chain from its highest opcode whose original tail byte is 00 / ff
 * (device/e8e9_forward_kernel.h).  max_steps: after that many serial steps a lane gives its buffer up (0: the engine's 2^20).
 * status[b]: 0 -- data[b] holds, byte for byte, what zpq_e8e9 makes of it; 1 declined -- data[b] is untouched and the caller
 * runs zpq_e8e9.  ZPQ_E_UNSUPPORTED with a note in zpq_last_error, and nothing touched, without a device or outside the range:
 * 65 535 buffers and 2 GiB per batch; the buffers, 8 bytes per 4 KiB and 4 bytes per seed and per chain within the device
 * budget. */
int zpq_e8e9_device(uint8_t* const* data, const uint32_t* len, uint32_t n, uint32_t max_steps, int32_t* status);
/* Blocks of this process's last zpq_compress_blocks call whose E8E9 filter (e8e9, libzpaq.cpp:6450-6459) ran on the device.  A
 * block qualifies when its method has E8E9 in front of LZ77 or the BWT (x.,5 .. x.,7) and it takes one of the device routes of the
 * pre-processing stage: the batched suffix sort with the parse behind it, the batched hash-table parse, or the wide sort of one
 * block of 16 MiB and more.  The copy that was uploaded for that route is filtered there before the route reads it, and the
 * filtered bytes come down into the caller's buffer, which holds what the reference leaves there whichever side filtered.
 * ZPAQ_AMD_DEVICE_E8=0|1, read per call, forces that off or on for qualifying blocks; unset it is off: e8_forward_pays and
 * e8_forward_wide_pays turn it on only from sizes at which it was measured to win on every kind of data.  A
 * block whose walk exceeds the step cap (ZPAQ_AMD_E8_MAX_STEPS=<steps> lowers it: tests) is filtered by the host and not counted;
 * x.,4 blocks and batches below the routes' thresholds are always filtered by the host.  The archives are the same either way. */
uint32_t zpq_last_device_e8_blocks(void);
/* The generic route on its own: the PCOMP program `code` (the bytes without the two length bytes, ph and pm as in the block
 * header) over n raw streams on the device, one lane per stream (device/pcomp_kernel.h: the program is translated to HIP and
 * compiled at run time unless a code object for it is cached).  hint[b] = the expected size of output b or 0 (a segment's size
 * comment; may be null: all 0): it only sizes the first attempt, an output beyond it costs a second launch.  The batch is one
 * launch and shares its fate: status[b] is 0 for every stream -- out[b] holds, byte for byte, what zpq_pcomp_host makes of
 * stream b, outlen[b] its size -- or 1 for every stream: declined, nothing was written, outlen[b] is 0, zpq_last_error names the
 * reason and the caller runs the batch on the host.  Declined are: any stream on which the device program stopped with a status
 * (`error`, a path that leaves the program, the budget of 2^30 backward jumps per call), a hint or an output beyond 2^32 - 16
 * bytes, a batch beyond the device budget.  The device never gives a verdict on a program or a stream.  When an output does
 * not fit its buffer every size is reported and nothing is written (ZPQ_E_OVERFLOW).  ZPQ_E_UNSUPPORTED with a note in
 * zpq_last_error without a device, or when the program has no kernel (arrays beyond ph 28 / pm 30, a failed compile). */
int zpq_pcomp_device(const uint8_t* code, size_t codelen, int ph, int pm, const uint8_t* const* stream, const uint32_t* len,
                     uint32_t n, const uint64_t* hint, uint8_t* const* out, const size_t* cap, size_t* outlen, int32_t* status);
/* The host's INTERPRETER with the same program over one stream, then the end-of-segment call: what zpq_decompress gives for a
 * block of one segment that carries the program, with the same errors (ZPQ_E_VM: `error`, an undefined instruction, leaving the
 * program, the step limit of zpq_set_pcomp_step_limit) -- also for a standard program, which zpq_decompress runs translated.
 * *outlen is the size also when the buffer is too small (ZPQ_E_OVERFLOW, nothing written). */
int zpq_pcomp_host(const uint8_t* code, size_t codelen, int ph, int pm, const uint8_t* in, uint32_t len, uint8_t* out, size_t cap,
                   size_t* outlen);
/* Segments of this process's last zpq_decompress call whose block's own PCOMP program ran on the device through that route: the
 * segments of blocks of one segment that carry a program, when the call holds 4 of them or 256 KiB (or ZPAQ_AMD_PCOMP=device),
 * less those another device decoder took and those of a group the device handed back. */
uint32_t zpq_last_device_pcomp_segments(void);
/* The archiver's fragmenting (zpaq.cpp `add`): every file is cut into content-defined fragments, each is hashed with SHA-1 and
 * the archiver deduplicates on the hash before it packs blocks.  zpq_fragment_limits: the smallest and largest fragment for
 * -fragment `fragment` (a negative one counts as 0) and the method's block size (2^(20 + N) - 4096; below 13 counts as 13).
 * zpq_fragment_host: the serial scan over n files.  nfrag[f] = the fragments of file f; then, for all fragments in order,
 * size[k], hits[k] (predictions of the fragment's order-1 table that held), sha1[20 k ..] and o1[256 k ..] (the table at the cut).
 * An empty file is one empty fragment; a file whose last byte is a cut ends with one more, empty, fragment; the SHA-1 of an
 * empty fragment is the SHA-1 of nothing.  *total = the fragments of the batch; when cap is smaller nothing else is written and
 * the call returns ZPQ_E_OVERFLOW.
 * zpq_fragment_device: the same results from the device (device/fragment_kernel.h): a wavefront walks each piece
 * of a file 64 positions at a time, the host stitches the pieces' lists where their cuts meet, SHA-1 runs per fragment on the
 * device.  ZPQ_E_UNSUPPORTED with a note in zpq_last_error without a device or outside the range: 65 535 files and 2 GiB per
 * batch, the files and their record lists (2 * 264 bytes per smallest fragment) within the device budget.  ZPAQ_AMD_FRAG_PIECE
 * (bytes, read per call) overrides the piece size of 256 KiB, or 64 smallest fragments where that is more (tests).  zpq_last_fragment_rounds: the fix-up rounds of this process's
 * last zpq_fragment_device call (0: every piece began at a cut; data that never re-joins, such as constant bytes, takes one
 * round per piece).
 * zpq_fragment_analyze: what the archiver computes for a fragment that did not deduplicate (zpaq.cpp:2436-2471) from its o1,
 * size and hits and the tables of the last four such fragments of the block, o1prev[4 * 256], oldest first, zero at the start of a
 * block: returns the final hits (the redundancy estimate), *text1 and *exe1 = 0 | 1.  The caller advances o1prev as the archiver
 * does (2530-2533): only behind a fragment of at least the smallest size, the four tables move down by one (the oldest leaves) and
 * the fragment's o1 becomes the last.  It runs on the host: which fragments deduplicate is the archiver's knowledge. */
void zpq_fragment_limits(int fragment, uint32_t blocksize, uint32_t* min_frag, uint32_t* max_frag);
int zpq_fragment_host(const uint8_t* const* in, const uint64_t* len, uint32_t n, int fragment, uint32_t blocksize,
                      uint32_t* nfrag /* [n] */, uint32_t* size, uint32_t* hits, uint8_t* sha1 /* 20 each */,
                      uint8_t* o1 /* 256 each */, size_t cap, size_t* total);
int zpq_fragment_device(const uint8_t* const* in, const uint64_t* len, uint32_t n, int fragment, uint32_t blocksize,
                        uint32_t* nfrag /* [n] */, uint32_t* size, uint32_t* hits, uint8_t* sha1 /* 20 each */,
                        uint8_t* o1 /* 256 each */, size_t cap, size_t* total);
uint32_t zpq_last_fragment_rounds(void);
uint32_t zpq_fragment_analyze(const uint8_t* o1 /* 256 */, uint64_t sz, uint32_t hits, const uint8_t* o1prev /* 1024 */,
                              int* text1, int* exe1);
void zpq_e8e9(uint8_t* data, uint32_t n);      /* e8e9 (libzpaq.cpp:6450-6459), in place */
/* Compiler alone (libzpaq.cpp:2698): ZPAQL source text -> header / PCOMP bytes. */
int zpq_assemble(const char* config, const int* args9, uint8_t* hcomp, size_t hcap,
                 size_t* hlen, uint8_t* pcomp, size_t pcap, size_t* plen);
/* Host copies of the predictor's constant tables (for tests): which = 0 squash
 * u16[4096], 1 stretch i16[32768], 2 dt i32[1024], 3 dt2k i32[256], 4 state
 * table u8[1024], 5 ICM initial side table u32[256], 6 ISSE initial side table
 * u32[512], 7 SSE initial row u32[32] (Predictor::init, libzpaq.cpp:1776-1846), 8 / 9 the compact form of
 * stretch the pipelined encoder keeps in LDS (u32[2016] groups of 8 + i16[256] top end).
 * Returns bytes written. */
size_t zpq_table(int which, void* out, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
