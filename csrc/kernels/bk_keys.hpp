// Order-preserving keys and the LDS digit count, shared by the order statistics
// (stats.hip: radix select, histogram) and the sort family (sort.hip).
#pragma once
#include "bk_common.hpp"

namespace bk {

constexpr int kPeel = 2;  // wave-combined indices before the per-lane atomics of lds_count

// hist[idx] += 1 for every lane with `on` set; idx is in bounds for those lanes.
// The LDS counts are u32 atomics.  A wave whose lanes all hit one counter
// (all-equal data; the top byte of uniform [0, 1) doubles) would serialise on
// that address, so the wave's most common indices are peeled first: the lanes
// that share the first active lane's index add their number once (__ballot +
// popcount), kPeel times over, and only what is left adds lane by lane.
// Every lane of a wave calls it together.
__device__ __forceinline__ void lds_count(unsigned* hist, unsigned idx, bool on) {
  const int lane = threadIdx.x & (kWave - 1);
  unsigned long long todo = __ballot(on);
#pragma unroll
  for (int it = 0; it < kPeel; ++it) {
    if (todo == 0ull) return;  // (wave-uniform: a ballot)
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned lead = (unsigned)__builtin_amdgcn_readlane((int)idx, leader);  // (leader: wave-uniform)
    const bool same = on && idx == lead;
    const unsigned long long peers = __ballot(same);
    if (lane == leader) atomicAdd(&hist[lead], (unsigned)__popcll(peers));
    todo &= ~peers;
    on = on && !same;
  }
  if (on) atomicAdd(&hist[idx], 1u);
}

// The order-preserving key of a float's bits (K: the unsigned integer of the
// dtype's size): negative values flipped whole, the others with the sign bit
// set, so unsigned key order is numeric order; every NaN, of either sign, maps
// to the largest key (numpy's sort puts NaNs last).  No other value has it.
template <typename K> struct Bits;
template <> struct Bits<uint64_t> { static constexpr uint64_t inf = 0x7ff0000000000000ull; };
template <> struct Bits<uint32_t> { static constexpr uint32_t inf = 0x7f800000u; };
template <> struct Bits<uint16_t> { static constexpr uint16_t inf = 0x7f80; };

template <typename K> __device__ __forceinline__ K to_key(K u) {
  constexpr K sign = (K)((K)1 << (8 * sizeof(K) - 1));
  if ((K)(u & (K)~sign) > Bits<K>::inf) return (K)~(K)0;
  return (u & sign) ? (K)~u : (K)(u | sign);
}
template <typename K> __device__ __forceinline__ K from_key(K k) {
  constexpr K sign = (K)((K)1 << (8 * sizeof(K) - 1));
  if (k == (K)~(K)0) return (K)(Bits<K>::inf | (Bits<K>::inf >> 1));  // a quiet NaN
  return (k & sign) ? (K)(k ^ sign) : (K)~k;
}

}  // namespace bk
