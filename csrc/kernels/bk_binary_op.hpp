// The binary arithmetic of bk_binary (elementwise.hip) and bk_broadcast
// (axis.hip): one definition, so an operand expanded by hand and the same
// operand broadcast by the kernel give the same bits.
#pragma once
#include "bk_common.hpp"

namespace bk {

enum BinaryOp : int { kBinAdd = 0, kBinSub, kBinMul, kBinDiv, kBinMax, kBinMin, kBinPow, kBinCount };

template <int OP, typename C>
__device__ __forceinline__ C binary(C a, C b) {
  if constexpr (OP == kBinAdd) return a + b;
  else if constexpr (OP == kBinSub) return a - b;
  else if constexpr (OP == kBinMul) return a * b;
  else if constexpr (OP == kBinDiv) return a / b;
  // numpy.maximum / minimum: NaN in either operand gives NaN
  else if constexpr (OP == kBinMax) return (a > b || a != a) ? a : b;
  else if constexpr (OP == kBinMin) return (a < b || a != a) ? a : b;
  else return pow(a, b);
}

}  // namespace bk
