// LZ77 streams back into their blocks on the MI355X, for streams long enough to be cut: the same contract as
// device/lz77_decode_kernel.h -- exactly what the method's PCOMP program makes of the stream, or declined -- with more than one
// chain per stream.  The format leaves no restart points, but the code stream re-synchronises by itself: a parse
// begun anywhere soon shares its code starts with the true one.  So:
//
//   unlzw_piece_kernel     one wavefront per PIECE of the stream (layout.h kUnlzWidePiece bytes): the parser of 4.5.3 started at
//                          the piece's first bit (level 1) or byte (level 2) as if a code began there, until a code starts at or
//                          behind the piece's end.  Tokens {out_pos relative to the piece, len, off, src} and, beside each, the
//                          state its code started in: the position relative to the piece and, at level 1, how far `t` (the call
//                          of the program the code starts in) is ahead of ceil(pos / 8) -- 0 .. 3 in any stream the parser takes.
//                          A provisional parse starts with t = ceil(pos / 8).  Two parses are in the same state only when both
//                          agree, and from there on they are the same to the stream's end, how it ends included.  What the
//                          parser refuses ends the piece's list quietly; the checks that need the absolute output position wait.
//   unlzw_stitch_kernel    one wavefront per stream, the pieces in order: piece k is entered in piece k - 1's true exit state.
//                          A code that leaps over the piece skips it.  Else the lanes look the state up in the piece's list
//                          (sorted by position, 64 entries per step); where it is found the list is adopted from there on, with
//                          its recorded exit; where not, ONE code is parsed serially into the stream's final list and the
//                          look-up repeats, until the walk has passed the piece's end.  Per piece it leaves {first adopted
//                          index, count, first final slot, output base}, per stream {out_len, ntok, status} and the counts.
//   unlzw_finalize_kernel  a lane per adopted token: the base added, the deferred checks (a match in front of the output's start,
//                          an output beyond 2^mbits), the token into the final list.  The first failing token of a stream, by
//                          index, leaves its status in the stream's error word (atomicMin).
//   -- the host reads 40 bytes per stream (the counts among them), places the outputs back to back and checks the room --
//   unlzw_link_kernel      a lane per output byte: the covering token by binary search; a literal's word is its byte with the top
//                          bit set, a match byte's the position it copies (p - off; in a run, off < len, the byte of the source
//                          period: out_pos - off + (p - out_pos) % off).
//   unlzw_jump_kernel      w[p] = w[w[p]] while w[p] is no literal, in place.  A word only ever moves to an ancestor, so any
//                          interleaving of lanes reaches the same fixed point; no lane waits for another.  A round that leaves a
//                          word unresolved raises the round's flag and the host launches the next (depth d: ceil(log2 d) rounds).
//   unlzw_emit_kernel      out[p] = the byte w[p] holds.
//   unlzw_emit_placed_kernel   the same bytes, each stream's at an offset of its own: the blocks as the inverse E8E9 filter takes
//                          them (device/e8e9_kernel.h), which runs behind this stage for the methods x.,5 and x.,6.
#pragma once
#include "lz77_decode_kernel.h"

namespace zpq {

enum { kUnlzwCode = 0, kUnlzwLast = 1, kUnlzwEnd = 2, kUnlzwErr = 3 };     // a step: a code; a code, then the stream ends; the end; refused

// One code of a level-1 stream in the program's own order of tests (unlz_parse_body has the same, inline): kUnlzwCode / kUnlzwLast
// leave the token {len, off (0: literals), src}, B and t behind the code.
__device__ __forceinline__ int unlzw_step_bits(UnlzBits& B, uint32_t& t, uint32_t n, uint32_t rb, uint32_t& len_o, uint32_t& off_o, uint32_t& src_o,
                                               uint32_t& status) {
  len_o = off_o = src_o = 0;
  if (t >= n) return kUnlzwEnd;
  if (8u * t - B.pos > 24u) { status = kUnlzField; return kUnlzwErr; }
  ++t;
  const uint32_t mm = B.get(2);
  uint32_t len = 1;
  if (mm) {
    const uint32_t r3 = (mm - 1u) * 8u + B.get(3);
    for (;;) {
      t = unlz_max(t, (B.pos + 3u + 7u) >> 3);
      if (t > n) return kUnlzwEnd;
      if (B.get(1)) {
        if (len >= (1u << 28)) { status = kUnlzField; return kUnlzwErr; }
        len = len * 2u + B.get(1);
      } else {
        len = len * 4u + B.get(2);
        break;
      }
    }
    uint32_t r5 = 0;
    if (rb) {
      t = unlz_max(t, (B.pos + rb + 7u) >> 3);
      if (t > n) return kUnlzwEnd;
      r5 = B.get(rb);
    }
    if (r3 > 24u) { status = kUnlzField; return kUnlzwErr; }
    t = unlz_max(t, (B.pos + r3 + 7u) >> 3);
    if (t > n) return kUnlzwEnd;
    uint32_t off = (1u << r3) | B.get(r3);
    if (rb) off = (off << rb) + r5 - ((1u << rb) - 1u);
    len_o = len;
    off_o = off;
    return kUnlzwCode;
  }
  for (;;) {
    t = unlz_max(t, (B.pos + 2u + 7u) >> 3);
    if (t > n) return kUnlzwEnd;
    if (!B.get(1)) break;
    if (len >= (1u << 28)) { status = kUnlzField; return kUnlzwErr; }
    len = len * 2u + B.get(1);
  }
  t = unlz_max(t, (B.pos + 8u + 7u) >> 3);
  if (t > n) return kUnlzwEnd;
  // one literal per call: the calls t .. n are there for them
  const uint32_t run = len, room = n - t + 1u, done = run < room ? run : room;
  len_o = done;
  src_o = B.pos;
  if (done < run) return kUnlzwLast;
  t += run - 1u;
  B.seek(B.pos + 8u * run);
  return kUnlzwCode;
}

// ... and of a level-2 stream; p: the byte the code starts at.  An offset of 2^32 (four bytes of 255) is stored as 2^32 - 1: either
// reaches in front of any output the decoder takes.  kUnlzwLast may leave no token (len 0: a run whose literals never arrived).
__device__ __forceinline__ int unlzw_step_bytes(UnlzWords& W, uint32_t& p, uint32_t n, uint32_t mmin, uint32_t& len_o, uint32_t& off_o, uint32_t& src_o,
                                                uint32_t& status) {
  len_o = off_o = src_o = 0;
  if (p >= n) return kUnlzwEnd;
  const uint32_t c = (W.word(p >> 2) >> (8u * (p & 3u))) & 255u;
  if (c < 64u) {
    const uint32_t run = c + 1u, room = n - (p + 1u), done = run < room ? run : room;
    len_o = done;
    src_o = p + 1u;
    if (done < run) return kUnlzwLast;
    p += 1u + run;
    return kUnlzwCode;
  }
  const uint32_t nb = (c >> 6) + 1u;
  if ((uint64_t)p + 1u + nb > n) return kUnlzwEnd;
  uint32_t o = 0;
  for (uint32_t k = 1; k <= nb; ++k) o = o << 8 | ((W.word((p + k) >> 2) >> (8u * ((p + k) & 3u))) & 255u);
  const uint32_t len = (c & 63u) + mmin;
  if (len == 0) { status = kUnlzEmpty; return kUnlzwErr; }
  len_o = len;
  off_o = o == 0xFFFFFFFFu ? o : o + 1u;
  p += 1u + nb;
  return kUnlzwCode;
}

// A walk over one stream of level 1 (kBits) or 2: pos() is where the next code starts, in bits or in bytes.  (The level is a
// template parameter so that a kernel keeps the state of one parser in registers, not of both.)
template <bool kBits>
struct UnlzwWalk {
  UnlzBits B;                    // level 1 (B.s: the stream's words, for either level)
  uint32_t rb, mmin, n;
  uint32_t p, t;                 // level 2: the byte cursor; level 1: the program's call
  __device__ __forceinline__ void init(const uint8_t* in_all, const UnlzWideStream& S, int lane) {
    B.s.w = (const uint32_t*)(in_all + S.in_off);
    B.s.nwords = (uint32_t)(((uint64_t)S.in_len + 3u) >> 2);
    B.s.lane = lane;
    B.s.load(0);
    rb = S.rb;
    mmin = S.min_match;
    n = S.in_len;
    p = t = 0;
    if (kBits) B.seek(0);
  }
  __device__ __forceinline__ uint32_t pos() const { return kBits ? B.pos : p; }
  __device__ __forceinline__ void enter(uint32_t at, uint32_t call) {
    if (kBits) { B.seek(at); t = call; } else p = at;
  }
  __device__ __forceinline__ int step(uint32_t& len, uint32_t& off, uint32_t& src, uint32_t& status) {
    if (kBits) return unlzw_step_bits(B, t, n, rb, len, off, src, status);
    return unlzw_step_bytes(B.s, p, n, mmin, len, off, src, status);
  }
  // the state of a code start inside a piece that starts at `start`: (relative position) << 2 | (t - ceil(pos / 8)); all ones
  // where t is further ahead than any code may start with (the step refuses it: 8t - pos > 24) -- the state of no list entry
  __device__ __forceinline__ uint32_t state(uint32_t start) const {
    if (!kBits) return (p - start) << 2;
    const uint32_t dt = t - ((B.pos + 7u) >> 3);
    return dt > 3u ? ~0u : (B.pos - start) << 2 | dt;
  }
};

// what the decoder takes at all (the same in every piece of a stream and in its stitch).  A batch is of one method: its kernels are
// instantiated for the level (kBits: level 1), and a stream of the other level is declined.
template <bool kBits>
__device__ __forceinline__ bool unlzw_in_range(const UnlzWideStream& S) {
  return kBits ? S.level == 1u && S.in_len < (1u << 29) && S.rb <= 7u : S.level == 2u && S.in_len < 0xFFF00000u;
}

// the parse of piece `index` of stream S into its slots
template <bool kBits>
__device__ __forceinline__ void unlzw_piece_walk(const uint8_t* in_all, const UnlzWideStream& S, uint32_t index, uint32_t piece, int lane, uint4* toks,
                                                 uint32_t* states, UnlzWidePieceOut& R) {
  const uint32_t unit = kBits ? 8u : 1u;
  const uint32_t first = index * piece, last = S.in_len - first < piece ? S.in_len : first + piece;      // bytes
  const uint32_t start = first * unit, end = last * unit;
  UnlzwWalk<kBits> W;
  W.init(in_all, S, lane);
  W.enter(start, first);
  uint64_t out = 0;
  uint32_t cnt = 0;
  uint4 mine;
  uint32_t smine = 0;
  mine.x = mine.y = mine.z = mine.w = 0;
  R.end = 0;
  R.status = kUnlzOk;
  while (W.pos() < end) {
    const uint32_t st = W.state(start);
    uint32_t len, off, src;
    const int r = W.step(len, off, src, R.status);
    if (r == kUnlzwErr) { R.end = 2u; break; }
    if (len) {
      // (an output of more than 2^31 bytes is beyond every mbits, wherever the piece's output starts)
      if (out + len > (1ull << 31)) { R.end = 2u; R.status = kUnlzLong; break; }
      if (cnt >= piece) { R.end = 2u; R.status = kUnlzFull; break; }
      if ((uint32_t)lane == (cnt & 63u)) { mine.x = (uint32_t)out; mine.y = len; mine.z = off; mine.w = src; smine = st; }
      ++cnt;
      if ((cnt & 63u) == 0) { toks[cnt - 64u + (uint32_t)lane] = mine; states[cnt - 64u + (uint32_t)lane] = smine; }
      out += len;
    }
    if (r != kUnlzwCode) { R.end = 1u; break; }
  }
  const uint32_t rem = cnt & 63u;
  if ((uint32_t)lane < rem) { toks[cnt - rem + (uint32_t)lane] = mine; states[cnt - rem + (uint32_t)lane] = smine; }
  R.codes = cnt;
  R.out_len = (uint32_t)out;
  R.exit_pos = W.pos();
  R.exit_t = W.t;
}

// (1) one wavefront per piece (64 threads per workgroup, blockIdx.x = the piece's index in refs)
template <bool kBits>
__device__ __forceinline__ void unlzw_piece_body(const uint8_t* in_all, const UnlzWideStream* streams, const UnlzWideRef* refs, uint32_t piece,
                                                 uint4* prov_all, uint32_t* states_all, UnlzWidePieceOut* pieces) {
  const uint32_t g = blockIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const UnlzWideRef ref = refs[g];
  const UnlzWideStream S = streams[ref.stream];
  const uint64_t slot0 = S.tok_off + (uint64_t)ref.index * piece;
  uint4* const toks = prov_all + slot0;
  uint32_t* const states = states_all + slot0;
  UnlzWidePieceOut R;
  R.codes = R.out_len = R.exit_pos = R.exit_t = 0;
  R.end = 2u;
  R.status = kUnlzField;
  if (unlzw_in_range<kBits>(S)) unlzw_piece_walk<kBits>(in_all, S, ref.index, piece, lane, toks, states, R);
  if (lane == 0) pieces[g] = R;
}

__device__ __forceinline__ unsigned long long unlzw_err_key(uint32_t tok, uint32_t status) { return (unsigned long long)tok << 3 | status; }
// the checks of a token that need its absolute position: 0, or the status it declines the stream with
__device__ __forceinline__ uint32_t unlzw_check(uint32_t out_pos, uint32_t len, uint32_t off, uint32_t max_out) {
  if (off && off > out_pos) return kUnlzBefore;
  if ((uint64_t)out_pos + len > max_out) return kUnlzLong;
  return kUnlzOk;
}

// what the stitch of a stream carries along
struct UnlzwTotals {
  uint32_t out_pos;              // (at most 2^31)
  uint32_t ntok, status;
};
template <bool kBits>
// (prov, states, pieces, fin, adopt: the stream's own)
__device__ __forceinline__ void unlzw_stitch_walk(const uint8_t* in_all, const UnlzWideStream& S, uint32_t piece, int lane, const uint4* prov,
                                                  const uint32_t* states_all, const UnlzWidePieceOut* pieces, uint4* fin, UnlzWideAdopt* adopt,
                                                  UnlzWideOut* out, UnlzwTotals& T) {
  const uint32_t max_out = S.mbits >= 31u ? (1u << 31) : (1u << S.mbits);
  const uint32_t cap = S.npieces * piece;                                // (unlzw_in_range: below 2^32)
  const uint32_t unit = kBits ? 8u : 1u;
  UnlzwWalk<kBits> W;
  W.init(in_all, S, lane);
  bool done = false;
  for (uint32_t k = 0; k < S.npieces && !done; ++k) {
    const uint32_t first = k * piece, last = S.in_len - first < piece ? S.in_len : first + piece;
    const uint32_t start = first * unit, end = last * unit;
    if (W.pos() >= end) continue;                                        // a code leapt over the piece
    const uint32_t codes = pieces[k].codes;                              // (the rest of the record is read where a list is adopted)
    const uint32_t* const states = states_all + first;
    uint32_t ci = 0, serial = 0;
    bool adopted = false;
    for (;;) {
      // the first entry of the piece's list at or behind the walk's position
      const uint32_t want = W.state(start);
      while (ci < codes) {
        const uint32_t i = ci + (uint32_t)lane;
        const uint32_t s = i < codes ? states[i] : ~0u;
        const unsigned long long m = __builtin_amdgcn_ballot_w64((s >> 2) >= (want >> 2));
        if (m) { ci += (uint32_t)__builtin_ctzll(m); break; }
        ci += 64u;
      }
      if (ci < codes && states[ci] == want) {                            // the same state: the list is the truth from here on
        const UnlzWidePieceOut P = pieces[k];
        const uint32_t at = prov[first + ci].x, count = codes - ci;
        if (count > cap - T.ntok) { T.status = kUnlzFull; done = true; break; }
        if (lane == 0) {
          UnlzWideAdopt A;
          A.first = ci; A.count = count; A.tok_base = T.ntok; A.out_base = T.out_pos - at;
          adopt[k] = A;
        }
        T.ntok += count;
        adopted = true;
        if (lane == 0) { if (serial) ++out->stats.met; else ++out->stats.entered; }
        if (P.out_len - at > (1u << 31) - T.out_pos) { T.status = kUnlzLong; done = true; break; }
        T.out_pos += P.out_len - at;
        if (P.end == 2u) { T.status = P.status; done = true; }
        else if (P.end == 1u) done = true;
        else W.enter(P.exit_pos, P.exit_t);
        break;
      }
      uint32_t len, off, src;
      const int r = W.step(len, off, src, T.status);
      if (r == kUnlzwErr) { done = true; break; }
      if (len) {
        const uint32_t bad = unlzw_check(T.out_pos, len, off, max_out);
        if (bad && lane == 0) atomicMin(&out->err, unlzw_err_key(T.ntok, bad));
        if (len > (1u << 31) - T.out_pos) { T.status = kUnlzLong; done = true; break; }
        if (T.ntok >= cap) { T.status = kUnlzFull; done = true; break; }
        if (lane == 0) { uint4 tk; tk.x = T.out_pos; tk.y = len; tk.z = off; tk.w = src; fin[T.ntok] = tk; }
        ++T.ntok;
        T.out_pos += len;
      }
      if (r != kUnlzwCode) { done = true; break; }
      ++serial;
      if (W.pos() >= end) break;
    }
    if (!adopted && lane == 0) ++out->stats.walked;                      // (to its end, or to the stream's)
  }
}

// (2) one wavefront per stream (64 threads per workgroup); `adopt` is zero when the kernel starts
template <bool kBits>
__device__ __forceinline__ void unlzw_stitch_body(const uint8_t* in_all, const UnlzWideStream* streams, uint32_t piece, const uint4* prov_all,
                                                  const uint32_t* states_all, const UnlzWidePieceOut* pieces, uint4* final_all, UnlzWideAdopt* adopt,
                                                  UnlzWideOut* outs) {
  const uint32_t b = blockIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const UnlzWideStream S = streams[b];
  uint4* const fin = final_all + S.tok_off;
  UnlzwTotals T;
  T.out_pos = 0;
  T.ntok = 0;
  T.status = kUnlzOk;
  if (lane == 0) {                                              // (lane 0 counts in memory: the walk's registers are scarce)
    outs[b].err = ~0ull;
    outs[b].stats.pieces = S.npieces;
    outs[b].stats.entered = outs[b].stats.met = outs[b].stats.walked = 0;
  }
  if (!unlzw_in_range<kBits>(S)) T.status = kUnlzField;
  else unlzw_stitch_walk<kBits>(in_all, S, piece, lane, prov_all + S.tok_off, states_all + S.tok_off, pieces + S.piece0, fin, adopt + S.piece0, outs + b, T);
  if (lane == 0) {
    UnlzResult r;
    r.out_len = T.out_pos;
    r.ntok = T.ntok;
    r.status = T.status;
    outs[b].r = r;
  }
}

// (3) a lane per adopted token: blockIdx.x = piece * chunks + chunk, chunks = (piece + 255) / 256 chunks of 256 tokens per piece
__device__ __forceinline__ void unlzw_finalize_body(const UnlzWideStream* streams, const UnlzWideRef* refs, uint32_t piece, const uint4* prov_all,
                                                    const UnlzWideAdopt* adopt, uint4* final_all, UnlzWideOut* outs) {
  const uint32_t chunks = (piece + 255u) / 256u;
  const uint32_t g = blockIdx.x / chunks, j = (blockIdx.x % chunks) * 256u + threadIdx.x;
  const UnlzWideAdopt A = adopt[g];
  if (j >= A.count) return;
  const UnlzWideRef ref = refs[g];                              // (also of a stream the stitch declined: an earlier token's status goes first)
  const UnlzWideStream S = streams[ref.stream];
  const uint32_t max_out = S.mbits >= 31u ? (1u << 31) : (1u << S.mbits);
  uint4 tk = prov_all[S.tok_off + (uint64_t)ref.index * piece + A.first + j];
  tk.x += A.out_base;
  const uint32_t bad = unlzw_check(tk.x, tk.y, tk.z, max_out);
  if (bad) atomicMin(&outs[ref.stream].err, unlzw_err_key(A.tok_base + j, bad));
  final_all[S.tok_off + A.tok_base + j] = tk;
}

// (4) a lane per output byte of the batch: place[0 .. nlive) are the decoded streams in the order of their outputs (none empty)
__device__ __forceinline__ void unlzw_link_body(const uint8_t* in_all, const UnlzWideStream* streams, const UnlzWidePlace* place, uint32_t nlive,
                                                uint32_t total, const uint4* final_all, uint32_t* w) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= total) return;
  uint32_t a = 0, z = nlive;                                    // the last stream whose output starts at or below q
  while (z - a > 1u) { const uint32_t mid = a + ((z - a) >> 1); if (place[mid].out_off <= q) a = mid; else z = mid; }
  const UnlzWidePlace L = place[a];
  const uint32_t p = q - (uint32_t)L.out_off;
  const UnlzWideStream S = streams[L.stream];
  const uint4* const toks = final_all + S.tok_off;
  uint32_t lo = 0, hi = L.ntok;                                 // the last token that starts at or below p
  while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (toks[mid].x <= p) lo = mid; else hi = mid; }
  const uint4 k = toks[lo];
  const uint32_t d = p - k.x, base = (uint32_t)L.out_off;
  uint32_t v;
  if (k.z == 0u) {
    const uint8_t* const in = in_all + S.in_off;
    if (S.level == 1u) {
      const uint32_t at = k.w + 8u * d, sh = at & 7u;
      v = in[at >> 3];
      if (sh) v = (v | (uint32_t)in[(at >> 3) + 1u] << 8) >> sh;
    } else v = in[k.w + d];
    v = (v & 255u) | 0x80000000u;
  } else if (k.z < k.y) v = base + k.x - k.z + d % k.z;
  else v = base + p - k.z;
  w[base + p] = v;
}

// (5) one round over the batch's `total` words; *flag = 1: some word is not resolved yet
__device__ __forceinline__ void unlzw_jump_body(uint32_t* w, uint32_t total, uint32_t* flag) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= total) return;
  const uint32_t v = w[p];
  if (v >> 31) return;
  const uint32_t u = w[v];
  w[p] = u;
  if (!(u >> 31)) *flag = 1u;
}

// (6)
__device__ __forceinline__ void unlzw_emit_body(const uint32_t* w, uint32_t total, uint8_t* out) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p < total) out[p] = (uint8_t)w[p];
}

// (6') ... for the inverse E8E9 filter behind this stage (device/e8e9_kernel.h): the words stay packed -- link and jump never see a
// gap -- and the bytes go where the filter wants its blocks, stream place[a]'s at dst_off[a] (a multiple of kE8Lane, the room
// behind it rounded up to one; the padding is not written).  A lane per packed byte q < total, the stream as unlzw_link_body finds it.
__device__ __forceinline__ void unlzw_emit_placed_body(const uint32_t* w, const UnlzWidePlace* place, const uint64_t* dst_off, uint32_t nlive,
                                                       uint32_t total, uint8_t* out) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= total) return;
  uint32_t a = 0, z = nlive;                                    // the last stream whose output starts at or below q
  while (z - a > 1u) { const uint32_t mid = a + ((z - a) >> 1); if (place[mid].out_off <= q) a = mid; else z = mid; }
  out[dst_off[a] + (q - (uint32_t)place[a].out_off)] = (uint8_t)w[q];
}

}  // namespace zpq
