// The wide suffix sort's kernels: ONE block of n bytes, 1 <= n < 2^31, one element per suffix (device/sa_kernels.hip holds the
// __global__ wrappers, the rocPRIM calls and the doubling loop).  The batched sorter (sa_kernel.h) spends 16 bits of its key on
// the block id and has 24 left for each rank; a block that is alone needs no id, so the key is two rank fields of r bits each,
// r = sa_wide_rank_bits(n) <= 31.
//
//   sa_wide_init_body     rank of round 0 (byte + 1)
//   sa_wide_keys_body     the round's key  rank[i] << w | rank[i + h]  (0 where i + h is past the end), w = sa_wide_field_bits(r, h)
//   (radix sort)          rocPRIM, on 2 w bits
//   sa_flags_body         (sa_kernel.h, as it is) 1 where a sorted key differs from its left neighbour
//   (inclusive scan)      rocPRIM
//   sa_wide_rename_body   new ranks = the scan: names start at 1, there is no block base to subtract
//   (sa_round_is_last decides on the host, unchanged)
//   sa_wide_invert_body   ranks -> suffix array
//   bwt_wide_body         ranks -> the BWT's last column in preprocess_block's layout, WITHOUT the array: the final rank of
//                         suffix i is its position in the array + 1, which is where its byte goes
//
// The field width is an argument, not a constant: a test runs a small string at the widths a large block would use.
#pragma once
#include "sa_kernel.h"

namespace zpq {

// smallest r with 2^r > n: ranks are 1..n, 0 means past the end
static inline unsigned sa_wide_rank_bits(uint64_t n) {
  unsigned r = 1;
  while ((1ull << r) <= n) ++r;
  return r;
}

// Width of one rank field in the round of step h.  Ranks of round 0 are byte + 1 (up to 256) whatever n is, so the first round
// needs 9 bits even where a block of fewer than 256 bytes has a narrower r; from the second round on ranks are names, at most n.
static inline unsigned sa_wide_field_bits(unsigned r, uint32_t h) { return h == 1 && r < 9 ? 9u : r; }

__device__ __forceinline__ void sa_wide_init_body(const uint8_t* in, uint32_t n, uint32_t* rank) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  rank[i] = (uint32_t)in[i] + 1u;
}

__device__ __forceinline__ void sa_wide_keys_body(const uint32_t* rank, uint32_t n, uint32_t h, uint32_t w, uint64_t* keys, uint32_t* vals) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t r2 = i + h < n ? rank[i + h] : 0u;
  keys[i] = (uint64_t)rank[i] << w | r2;
  vals[i] = (uint32_t)i;
}

// new rank of the element at sorted position j: the number of distinct keys up to and including its own
__device__ __forceinline__ void sa_wide_rename_body(const uint32_t* vals, const uint32_t* scan, uint32_t n, uint32_t* rank) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  rank[vals[j]] = scan[j];
}

// ranks are a permutation of 1..n now
__device__ __forceinline__ void sa_wide_invert_body(const uint32_t* rank, uint32_t n, uint32_t* sa) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  sa[rank[i] - 1u] = (uint32_t)i;
}

// BWT as preprocess_block lays it out (n + 1 bytes at out): out[0] = last byte, out[j + 1] = the byte in front of suffix sa[j],
// 255 for the whole string, whose 1-based index goes to idx[0].  Suffix i stands at j = rank[i] - 1, so every thread scatters
// the byte in front of its own suffix: both loads are coalesced and the array is never built.
__device__ __forceinline__ void bwt_wide_body(const uint8_t* in, const uint32_t* rank, uint32_t n, uint8_t* out, uint32_t* idx) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t at = rank[i];
  out[at] = i ? in[i - 1] : (uint8_t)255;
  if (i == 0) { idx[0] = at; out[0] = in[n - 1]; }
}

}  // namespace zpq
