// The batched suffix sort's kernels (device/sa_kernels.hip holds the __global__ wrappers, the rocPRIM calls and the doubling
// loop; the algorithm is described there): one element per suffix of every block of the batch, block b owns [off[b], off[b + 1]).
//
//   sa_init_body     rank of round 0 (byte + 1) and the block of every element
//   sa_keys_body     the round's key  block << 48 | rank[i] << 24 | rank[i + h]  (0 where i + h is past the END OF THE BLOCK)
//   (radix sort)     rocPRIM, on sa_key_bits(nblocks) bits
//   sa_flags_body    1 where a sorted key differs from its left neighbour
//   (inclusive scan) rocPRIM
//   sa_rename_body   new ranks, counted from the block's first sorted element
//   (sa_round_is_last decides on the host whether another round follows)
//   sa_invert_body   ranks -> suffix array
//
// The bodies and the loop's two decisions live here so that the emulator runs this file, not a restatement of it
// (tests/emu/sa_emu_main.cpp: the library calls replaced by std::stable_sort on the masked key and std::partial_sum).
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

namespace zpq {

// The loop's two decisions, made on the host.  Bits of the key that matter to the sort: the block id on top of two 24-bit ranks
static inline unsigned sa_key_bits(uint32_t nblocks) {
  unsigned blk_bits = 1;
  while ((1u << blk_bits) < nblocks) ++blk_bits;
  return 48 + blk_bits;
}

// after the round of step h: `names` = the last prefix sum.  Every key distinct <=> it equals the number of elements.  A round
// with 2h >= max_len compares whole suffixes, so the names are distinct one round before h reaches max_len: the second test
// bounds the rounds whatever the names say (1 + ceil(log2(max_len)) at the most), it does not end a healthy sort.
static inline bool sa_round_is_last(uint64_t names, uint64_t total, uint32_t h, uint32_t max_len) {
  return names == total || h >= max_len;
}

// rank of round 0: byte + 1 (1..256); block id and position of every element
__device__ __forceinline__ void sa_init_body(const uint8_t* const* in, const uint64_t* off, uint32_t nblocks, uint64_t total, uint32_t* rank,
                                             uint16_t* blk) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  // block of element i: binary search in off[0..nblocks]
  uint32_t lo = 0, hi = nblocks;
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (off[mid] <= i) lo = mid; else hi = mid; }
  blk[i] = (uint16_t)lo;
  rank[i] = (uint32_t)in[lo][i - off[lo]] + 1u;
}

__device__ __forceinline__ void sa_keys_body(const uint32_t* rank, const uint16_t* blk, const uint64_t* off, uint64_t total, uint32_t h,
                                             uint64_t* keys, uint32_t* vals) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const uint32_t b = blk[i];
  const uint64_t end = off[b + 1];
  const uint32_t r2 = i + h < end ? rank[i + h] : 0u;
  keys[i] = (uint64_t)b << 48 | (uint64_t)rank[i] << 24 | r2;
  vals[i] = (uint32_t)i;
}

// 1 where a sorted key differs from its left neighbour (the first element of the array counts as different)
__device__ __forceinline__ void sa_flags_body(const uint64_t* keys, uint64_t total, uint32_t* flags) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= total) return;
  flags[j] = (j == 0 || keys[j] != keys[j - 1]) ? 1u : 0u;
}

// new rank of the element at sorted position j: names counted from the block's first sorted position (= off[block]: the
// block id is the major key), starting at 1
__device__ __forceinline__ void sa_rename_body(const uint64_t* keys, const uint32_t* vals, const uint32_t* scan, const uint64_t* off, uint64_t total,
                                               uint32_t* rank) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= total) return;
  const uint32_t b = (uint32_t)(keys[j] >> 48);
  rank[vals[j]] = scan[j] - scan[off[b]] + 1u;
}

// ranks are a permutation of 1..n_b inside every block now: sa[off_b + rank - 1] = position in the block
__device__ __forceinline__ void sa_invert_body(const uint32_t* rank, const uint16_t* blk, const uint64_t* off, uint64_t total, uint32_t* sa) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const uint64_t o = off[blk[i]];
  sa[o + rank[i] - 1u] = (uint32_t)(i - o);
}

}  // namespace zpq
