// The archiver's content-defined fragments on the MI355X -- what host/fragment.cpp fragment_scan computes, for a batch of files
// that lie in one device buffer.  Per fragment the scan keeps an order-1 table o1[256], the previous byte c1, a 32-bit hash h and
// a count of hits; byte c is a hit when c == o1[c1], then h = (h + c + 1) * (hit ? 314159265 : 271828182), o1[c1] = c, c1 = c.
// A cut lies behind a byte when the fragment has max_frag bytes, or h < thresh and it has min_frag; everything resets there.
// It looks byte-serial and is not:
//
//   - inside a STEP of 64 positions, a lane each: the context of a lane is the byte in front of it (the carried c1 for lane 0).
//     Its prediction is the byte of the nearest lower lane with the same context -- that lane's store is the last one into
//     o1[context] in front of it -- and o1[context] as the step found it when there is none.  Eight ballots over the context's
//     bits give the lanes with an equal context, as in device/bwt_decode_kernel.h;
//   - a position is the affine map x -> A x + B mod 2^32 with A one of the two multipliers and B = (c + 1) A.  Maps compose, so
//     an inclusive scan over the lanes (six DPP rounds: row shifts, then the rows folded) gives every lane's h from the step's h;
//   - a ballot of the cut condition gives the first cut lane L.  o1 takes the stores of lanes <= L only (of equal contexts the
//     highest lane's), hits counts those, the record is written, and the next step begins at L + 1 with a fresh state.  Without
//     a cut the step carries h, c1 and the size on.
//
// frag_walk_kernel: a wavefront (a workgroup of 64) per job.  It walks from job.start as if a cut lay in front of it, appends a
// record per fragment -- end, hits, the table as 64 words -- and ends at the first cut at or beyond job.stop, at a cut that is
// found in the job's merge list (two walks with a cut in common are the same from there on: the state resets), or at the end of
// file, where the fragment that ran into it is recorded too (it may be empty).  o1 lives in LDS, 256 bytes.  Every step consumes
// at least one byte or ends the walk, so the loop is bounded by the bytes left in the file; the merge cursor only moves
// forward.  No wavefront waits for another and nothing spins on memory.  The 64 bytes behind a step are loaded while the step is
// worked out; behind a cut the next step's bytes are shuffled together from the two loads.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "layout.h"

namespace zpq {

__device__ __forceinline__ void frag_emit(FragRec* r, uint32_t end, uint32_t hits, uint32_t lane, uint32_t word) {
  if (lane == 0u) { r->end = end; r->hits = hits; }
  ((uint32_t*)r->o1)[lane] = word;
}

// lane's map after the map of the lane the DPP control names (the identity where it names none): self o lower
template <int kCtrl, int kRows>
__device__ __forceinline__ void frag_compose(uint32_t& A, uint32_t& B) {
  const uint32_t a = (uint32_t)__builtin_amdgcn_update_dpp(1, (int)A, kCtrl, kRows, 0xF, false);
  const uint32_t b = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)B, kCtrl, kRows, 0xF, false);
  B = A * b + B;
  A = A * a;
}

__device__ __forceinline__ void frag_walk_body(const uint8_t* buf, const FragJob* jobs, uint32_t njobs, FragParams P, FragRec* recs,
                                               FragResult* res) {
  __shared__ uint32_t o1w[64];
  uint8_t* const o1 = (uint8_t*)o1w;
  const uint32_t g = blockIdx.x, lane = threadIdx.x & 63u;
  if (g >= njobs) return;
  const FragJob J = jobs[g];
  const uint8_t* const d = buf + J.off;
  FragRec* const out = recs + J.rec_off;
  const FragRec* const mlist = recs + J.merge_off;
  const unsigned long long below = (1ull << lane) - 1ull, self = 1ull << lane;
  o1w[lane] = 0u;
  __syncthreads();
  uint32_t p = J.start, sz = 0, hits = 0, h = 0, c1 = 0, count = 0, mi = 0, status = (uint32_t)kFragStop;
  uint32_t c = p < J.n && lane < J.n - p ? (uint32_t)d[p + lane] : 0u;      // byte p + lane, 0 behind the end of file
  for (;;) {
    if (p >= J.n) {                                             // the fragment that ran into the end of file
      if (count >= J.rec_cap) { status = (uint32_t)kFragFull; break; }
      frag_emit(out + count, J.n, hits, lane, o1w[lane]);
      ++count;
      status = (uint32_t)kFragEof;
      break;
    }
    const uint32_t left = J.n - p, nv = left < 64u ? left : 64u;
    const bool valid = lane < nv;
    const uint32_t pn = p + 64u;
    const uint32_t cn = pn < J.n && lane < J.n - pn ? (uint32_t)d[pn + lane] : 0u;      // the step behind, on its way
    uint32_t ctx = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)c, 0x138, 0xF, 0xF, false);   // wave_shr:1
    if (lane == 0u) ctx = c1;
    unsigned long long same = __builtin_amdgcn_ballot_w64(valid);
    for (uint32_t k = 0; k < 8u; ++k) {
      const bool bit = (ctx >> k) & 1u;
      const unsigned long long m = __builtin_amdgcn_ballot_w64(bit);
      same &= bit ? m : ~m;
    }
    const unsigned long long before = same & below;
    const uint32_t src = before ? 63u - (uint32_t)__builtin_clzll(before) : lane;
    const uint32_t cs = __shfl(c, (int)src);
    const uint32_t pred = before ? cs : (uint32_t)o1[ctx];
    const bool hit = valid && c == pred;
    uint32_t A = hit ? 314159265u : 271828182u, B = (c + 1u) * A;
    if (!valid) { A = 1u; B = 0u; }
    frag_compose<0x111, 0xF>(A, B);                             // row_shr:1, 2, 4, 8: the maps of the lanes below it in the row
    frag_compose<0x112, 0xF>(A, B);
    frag_compose<0x114, 0xF>(A, B);
    frag_compose<0x118, 0xF>(A, B);
    frag_compose<0x142, 0xA>(A, B);                             // row_bcast:15 into rows 1 and 3
    frag_compose<0x143, 0xC>(A, B);                             // row_bcast:31 into rows 2 and 3
    const uint32_t hk = A * h + B, szk = sz + lane + 1u;
    const bool cut = valid && (szk >= P.max_frag || (hk < P.thresh && szk >= P.min_frag));
    const unsigned long long cm = __builtin_amdgcn_ballot_w64(cut), hm = __builtin_amdgcn_ballot_w64(hit);
    const uint32_t last = cm ? (uint32_t)__builtin_ctzll(cm) : nv - 1u;
    const unsigned long long upto = last >= 63u ? ~0ull : (2ull << last) - 1ull;
    __syncthreads();                                            // (every lane has read its prediction)
    if (valid && lane <= last && !(same & ~below & ~self & upto)) o1[ctx] = (uint8_t)c;
    hits += (uint32_t)__builtin_popcountll(hm & upto);
    __syncthreads();
    if (cm) {
      const uint32_t end = p + last + 1u;
      if (count >= J.rec_cap) { status = (uint32_t)kFragFull; break; }
      frag_emit(out + count, end, hits, lane, o1w[lane]);
      ++count;
      o1w[lane] = 0u;                                           // (the word the lane has just read itself)
      __syncthreads();
      p = end; sz = 0u; hits = 0u; h = 0u; c1 = 0u;
      const uint32_t fromc = __shfl(c, (int)((lane + last + 1u) & 63u)), fromn = __shfl(cn, (int)((lane + last + 1u) & 63u));
      c = lane + last + 1u < 64u ? fromc : fromn;
      if (end < J.n) {                                          // (a cut at n goes on: the empty fragment behind it is recorded)
        if (J.merge_cnt) {
          while (mi < J.merge_cnt && mlist[mi].end < end) ++mi;
          if (mi < J.merge_cnt && mlist[mi].end == end) { status = (uint32_t)kFragMerged; break; }
        }
        if (end >= J.stop) { status = (uint32_t)kFragStop; break; }
      }
    } else {
      h = (uint32_t)__builtin_amdgcn_readlane((int)hk, (int)(nv - 1u));
      c1 = (uint32_t)__builtin_amdgcn_readlane((int)c, (int)(nv - 1u));
      sz += nv;
      p += nv;
      c = cn;
    }
  }
  if (lane == 0u) { FragResult r; r.count = count; r.status = status; r.merge_at = mi; res[g] = r; }
}

}  // namespace zpq
