// LZ77 streams back into their blocks on the MI355X -- what the PCOMP programs of the LZ77 methods without E8E9 compute
// (host/method.cpp pcomp_lz77_bits / pcomp_lz77_bytes, run by host/postproc.cpp), for a batch of streams, a wavefront per stream.
// The formats are the ones device/lz77_codes_kernel.h writes: level 1 bit-packed, least significant bit first,
// level 2 byte-aligned.
//
// Only FINDING the codes is a chain, and it is a chain per code, not per byte:
//
//   unlz_parse_kernel   one wavefront per stream, the state wave-uniform (the bit position or byte cursor, the output position
//                       as a running sum, the number of tokens): the stream is read 64 words at a time, one per lane, and every
//                       code appends one 16-byte token {out_pos, len, off (0 = literals), src}; src = the bit (level 1) or byte
//                       (level 2) position of a run's first literal.  Tokens are gathered 64 to a register (lane = token & 63)
//                       and stored with one coalesced store.  A match that continues the one before it at the same offset --
//                       the pieces level 2 cuts a long match into -- extends that token: the same copy.  At the end lane 0
//                       stores {out_len, ntok, status}.
//   -- the host reads the 12 bytes per stream, places the outputs back to back and checks the room --
//   unlz_copy_kernel    one wavefront per stream; tokens in windows of 64 (lane = token, staged in LDS).  A GROUP is the longest
//                       prefix of what is left of the window in which every token behind the first has its source final before
//                       the group starts: out_pos - off + min(len, off) <= out_pos(first).  One ballot finds it.  Then
//                       lane = output byte in steps of 64: the covering token by binary search over the window (6 steps), a
//                       literal from the stream, a match byte from out[p - off], a run (off < len) from
//                       out[out_pos - off + (p - out_pos) % off].  Nothing a group reads lies in what it writes, so the result
//                       does not depend on the order of lanes; one workgroup-scope release / acquire per group makes the
//                       wavefront's stores visible to its next loads.
//
// How a stream ENDS is the program's, exactly.  The program is called once per input byte and does a bounded amount per call:
// level 1 adds 8 bits to its buffer, starts at most one code (only when none is open), and emits at most one literal byte; a
// field is read only once the buffer holds enough bits (the program's own tests: more than 2 bits for a step of a match's length,
// more than 1 for a step of a run's, rb, the offset's bits, 8 for a literal).  The parser carries `t`, the call the program would
// be in, beside the bit position: a field that the call of the last byte cannot read never happens, a run keeps the literals whose
// calls happened.  Level 2 reads a byte per call: an unfinished match is dropped, a run keeps what arrived.
//
// status != 0: DECLINED -- the stream goes down the route the caller had before, its output is untouched:
//   1  a match reaches in front of the output's start (the program would read its circular M there)
//   2  a match of length 0 (level 2 with a minimum match of 0: the program's copy loop would wrap)
//   3  the output would exceed 2^mbits bytes (M wraps there)
//   4  the token list is full
//   5  a field the program's 32-bit registers would not hold: offset bits beyond 24, a length beyond 2^28, a stream of 2^29
//      bytes or more at level 1, a bit buffer of more than 24 bits at the start of a call
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "layout.h"

namespace zpq {

__device__ __forceinline__ void unlz_group_fence() {
#ifdef ZPQ_EMU
  (void)emu::wave_exchange(0);                     // every lane's stores are done before any lane goes on
#else
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#endif
}

// The stream as 32-bit words, 64 at a time: lane l holds word base + l of the chunk in use (0 behind the stream's last word).
struct UnlzWords {
  const uint32_t* w;
  uint32_t nwords, base, mine;
  int lane;
  __device__ __forceinline__ void load(uint32_t chunk_base) {
    base = chunk_base;
    const uint32_t i = base + (uint32_t)lane;
    mine = i < nwords ? w[i] : 0u;
  }
  __device__ __forceinline__ uint32_t word(uint32_t i) {          // i is the same in every lane
    if ((i & ~63u) != base) load(i & ~63u);
    return (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)(i & 63u));
  }
};

// bits of a level-1 stream, least significant first
struct UnlzBits {
  UnlzWords s;
  uint64_t buf;
  uint32_t have, next, pos;      // bits in buf, the next word to take, the position of buf's first bit
  __device__ __forceinline__ void seek(uint32_t p) {
    pos = p;
    next = (p >> 5) + 1u;
    buf = (uint64_t)s.word(p >> 5) >> (p & 31u);
    have = 32u - (p & 31u);
  }
  __device__ __forceinline__ uint32_t get(uint32_t k) {           // k <= 24
    if (have < k) { buf |= (uint64_t)s.word(next++) << have; have += 32u; }
    const uint32_t v = (uint32_t)buf & ((1u << k) - 1u);
    buf >>= k;
    have -= k;
    pos += k;
    return v;
  }
};

// the list a parse appends to: 64 tokens to a register, one coalesced store per 64
struct UnlzList {
  uint4* toks;
  uint32_t cap, n;
  uint4 mine, pend;
  bool open;                     // pend holds a token that a match may still extend
  int lane;
  __device__ __forceinline__ bool put(const uint4& t) {
    if (n >= cap) return false;
    if ((uint32_t)lane == (n & 63u)) mine = t;
    ++n;
    if ((n & 63u) == 0) toks[n - 64u + (uint32_t)lane] = mine;
    return true;
  }
  __device__ __forceinline__ bool add(uint32_t out_pos, uint32_t len, uint32_t off, uint32_t src) {
    if (open && off && pend.z == off) { pend.y += len; return true; }
    if (open && !put(pend)) return false;
    pend.x = out_pos; pend.y = len; pend.z = off; pend.w = src;
    open = true;
    return true;
  }
  __device__ __forceinline__ bool finish() {
    if (open && !put(pend)) return false;
    open = false;
    const uint32_t rem = n & 63u;
    if ((uint32_t)lane < rem) toks[n - rem + (uint32_t)lane] = mine;
    return true;
  }
};

__device__ __forceinline__ uint32_t unlz_max(uint32_t a, uint32_t b) { return a > b ? a : b; }

// (a) one wavefront per stream (64 threads per workgroup)
__device__ __forceinline__ void unlz_parse_body(const uint8_t* in_all, const UnlzStream* streams, uint4* toks_all, UnlzResult* res) {
  const uint32_t b = blockIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const UnlzStream S = streams[b];
  const uint32_t n = S.in_len;
  const uint64_t max_out = S.mbits >= 31u ? (1ull << 31) : (1ull << S.mbits);
  UnlzList L;
  L.toks = toks_all + S.tok_off;
  L.cap = S.tok_cap;
  L.n = 0;
  L.open = false;
  L.lane = lane;
  L.mine.x = L.mine.y = L.mine.z = L.mine.w = 0;
  L.pend = L.mine;
  UnlzWords W;
  W.w = (const uint32_t*)(in_all + S.in_off);
  W.nwords = (uint32_t)(((uint64_t)n + 3u) >> 2);
  W.lane = lane;
  W.load(0);
  uint64_t out_pos = 0;
  uint32_t status = kUnlzOk;
  if (S.level == 1) {
    UnlzBits B;
    B.s = W;
    B.seek(0);
    const uint32_t rb = S.rb;
    uint32_t t = 0;                               // calls of the program so far: bytes it has been given
    if (n >= (1u << 29) || rb > 7u) status = kUnlzField;
    while (status == kUnlzOk) {
      // a new code starts in the call behind the one that finished the last
      if (t >= n) break;
      if (8u * t - B.pos > 24u) { status = kUnlzField; break; }
      ++t;
      uint32_t mm, r3 = 0, len = 1;
      bool cut = false;
      {
        mm = B.get(2);
        if (mm) {
          r3 = (mm - 1u) * 8u + B.get(3);
          for (;;) {
            t = unlz_max(t, (B.pos + 3u + 7u) >> 3);
            if (t > n) { cut = true; break; }
            if (B.get(1)) {
              if (len >= (1u << 28)) { status = kUnlzField; break; }
              len = len * 2u + B.get(1);
            } else {
              len = len * 4u + B.get(2);
              break;
            }
          }
        } else {
          for (;;) {
            t = unlz_max(t, (B.pos + 2u + 7u) >> 3);
            if (t > n) { cut = true; break; }
            if (!B.get(1)) break;
            if (len >= (1u << 28)) { status = kUnlzField; break; }
            len = len * 2u + B.get(1);
          }
        }
      }
      if (mm) {
        if (cut || status != kUnlzOk) break;
        uint32_t r5 = 0;
        if (rb) {
          t = unlz_max(t, (B.pos + rb + 7u) >> 3);
          if (t > n) break;
          r5 = B.get(rb);
        }
        if (r3 > 24u) { status = kUnlzField; break; }
        t = unlz_max(t, (B.pos + r3 + 7u) >> 3);
        if (t > n) break;
        uint32_t off = (1u << r3) | B.get(r3);
        if (rb) off = (off << rb) + r5 - ((1u << rb) - 1u);
        if ((uint64_t)off > out_pos) { status = kUnlzBefore; break; }
        if (out_pos + len > max_out) { status = kUnlzLong; break; }
        if (!L.add((uint32_t)out_pos, len, off, 0u)) { status = kUnlzFull; break; }
        out_pos += len;
      } else {
        const uint32_t run = len;
        if (cut || status != kUnlzOk) break;
        t = unlz_max(t, (B.pos + 8u + 7u) >> 3);
        if (t > n) break;
        // one literal per call: the calls t .. n are there for them
        const uint32_t room = n - t + 1u, done = run < room ? run : room;
        if (out_pos + done > max_out) { status = kUnlzLong; break; }
        if (!L.add((uint32_t)out_pos, done, 0u, B.pos)) { status = kUnlzFull; break; }
        out_pos += done;
        if (done < run) break;
        t += run - 1u;
        B.seek(B.pos + 8u * run);
      }
    }
  } else {
    const uint32_t mmin = S.min_match;
    uint32_t p = 0;
    while (p < n) {
      const uint32_t c = (W.word(p >> 2) >> (8u * (p & 3u))) & 255u;
      if (c < 64u) {
        const uint32_t run = c + 1u, room = n - (p + 1u), done = run < room ? run : room;
        if (done) {
          if (out_pos + done > max_out) { status = kUnlzLong; break; }
          if (!L.add((uint32_t)out_pos, done, 0u, p + 1u)) { status = kUnlzFull; break; }
          out_pos += done;
        }
        if (done < run) break;
        p += 1u + run;
      } else {
        const uint32_t nb = (c >> 6) + 1u;
        if ((uint64_t)p + 1u + nb > n) break;
        uint32_t o = 0;
        for (uint32_t k = 1; k <= nb; ++k) o = o << 8 | ((W.word((p + k) >> 2) >> (8u * ((p + k) & 3u))) & 255u);
        const uint64_t off = (uint64_t)o + 1u;
        const uint32_t len = (c & 63u) + mmin;
        if (len == 0) { status = kUnlzEmpty; break; }
        if (off > out_pos) { status = kUnlzBefore; break; }
        if (out_pos + len > max_out) { status = kUnlzLong; break; }
        if (!L.add((uint32_t)out_pos, len, (uint32_t)off, 0u)) { status = kUnlzFull; break; }
        out_pos += len;
        p += 1u + nb;
      }
    }
    if (S.level != 2) status = kUnlzField;
  }
  if (status == kUnlzOk && !L.finish()) status = kUnlzFull;
  if (lane == 0) {
    UnlzResult r;
    r.out_len = (uint32_t)out_pos;
    r.ntok = L.n;
    r.status = status;
    res[b] = r;
  }
}

// (c) one wavefront per stream (64 threads per workgroup); out_off[b] = the first byte of stream b's output in out_all
__device__ __forceinline__ void unlz_copy_body(const uint8_t* in_all, const UnlzStream* streams, const uint4* toks_all, const UnlzResult* res,
                                               const uint64_t* out_off, uint8_t* out_all) {
  __shared__ uint4 win[64];
  const uint32_t b = blockIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const UnlzStream S = streams[b];
  const UnlzResult R = res[b];
  if (R.status != kUnlzOk || R.ntok == 0) return;            // (the same in every lane)
  const uint8_t* in = in_all + S.in_off;
  const uint4* toks = toks_all + S.tok_off;
  uint8_t* out = out_all + out_off[b];
  const bool bits = S.level == 1;
  for (uint32_t wbase = 0; wbase < R.ntok; wbase += 64u) {
    const uint32_t nwin = R.ntok - wbase < 64u ? R.ntok - wbase : 64u;
    uint4 tk;
    tk.x = tk.y = tk.z = tk.w = 0;
    if ((uint32_t)lane < nwin) tk = toks[wbase + (uint32_t)lane];
    __syncthreads();                                          // (the window before this one has been read)
    win[lane] = tk;
    __syncthreads();
    uint32_t g = 0;
    while (g < nwin) {
      const uint32_t gstart = win[g].x;
      // the first token behind g whose source is not final yet (or the end of the window) ends the group
      const uint32_t reach = tk.x - tk.z + (tk.y < tk.z ? tk.y : tk.z);
      const bool stop = (uint32_t)lane > g && ((uint32_t)lane >= nwin || (tk.z != 0u && reach > gstart));
      const unsigned long long m = __builtin_amdgcn_ballot_w64(stop);
      const uint32_t e = m ? (uint32_t)__builtin_ctzll(m) : 64u;
      const uint32_t gend = win[e - 1u].x + win[e - 1u].y;
      for (uint32_t p = gstart + (uint32_t)lane; p < gend; p += 64u) {
        uint32_t lo = g, hi = e;                              // the last token of the group that starts at or below p
        while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (win[mid].x <= p) lo = mid; else hi = mid; }
        const uint4 k = win[lo];
        const uint32_t d = p - k.x;
        uint32_t v;
        if (k.z == 0u) {
          if (bits) {
            const uint32_t at = k.w + 8u * d, sh = at & 7u;
            v = in[at >> 3];
            if (sh) v = (v | (uint32_t)in[(at >> 3) + 1u] << 8) >> sh;
          } else v = in[k.w + d];
        } else if (k.z < k.y) v = out[k.x - k.z + d % k.z];
        else v = out[p - k.z];
        out[p] = (uint8_t)v;
      }
      unlz_group_fence();
      g = e;
    }
  }
}

}  // namespace zpq
