// Run-time codes -> template arguments, written once: an op code, a flag or a
// dtype code picks the one instantiation a launch needs.  The callee is a
// generic lambda that takes the value as a tag type and returns a status:
//
//   return dispatch_dtype<float, double>(dtype, [&](auto t) {
//     using T = typename decltype(t)::type;
//     return dispatch_op<kCount>(op, [&](auto opc) {
//       constexpr int OP = decltype(opc)::value;
//       return dispatch_flag(big, [&](auto nt) {
//         kernel<T, OP, decltype(nt)::value><<<...>>>(...);
//         return launch_status();
//       });
//     });
//   });
//
// A code outside the range or the list is kBadArgument and calls nothing.
// Every (type, op, flag) combination the lambda's body names is instantiated:
// keep combinations nobody launches behind `if constexpr`.
//
// Plain C++: nothing here needs hipcc (tests/dispatch_main.cpp is built by g++).
#pragma once
#include <type_traits>
#include <utility>

namespace bk {

enum Status : int {
  kOk = 0,
  kBadArgument = 1,
  kLaunchFailed = 2,
  kOutOfMemory = 3,
  kQuotaExceeded = 4,
  kNotInitialized = 5,
};

// kBool: numpy's bool, one byte per element -- kernels write exactly 0 or 1
// and read any non-zero byte as true (mask.hip)
enum DType : int { kF32 = 0, kF64 = 1, kBF16 = 2, kF16 = 3, kI32 = 4, kI64 = 5, kBool = 6 };

template <typename F, int... IS>
int dispatch_op_in(int op, F&& f, std::integer_sequence<int, IS...>) {
  int rc = kBadArgument;
  ((op == IS ? (rc = f(std::integral_constant<int, IS>{}), 0) : 0), ...);
  return rc;
}
// f(std::integral_constant<int, op>{}) for op in [0, COUNT)
template <int COUNT, typename F>
int dispatch_op(int op, F&& f) {
  return dispatch_op_in(op, f, std::make_integer_sequence<int, COUNT>{});
}

// f(std::true_type{}) or f(std::false_type{})
template <typename F>
int dispatch_flag(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}

// The element type a kernel is instantiated with for a dtype code (bf16 moves
// as its 16 bits, a bool as its byte: uint16_t and uint8_t, spelled without
// <stdint.h>).  The only place the map is written.
template <typename T> struct DTypeOf;
template <> struct DTypeOf<float> : std::integral_constant<int, kF32> {};
template <> struct DTypeOf<double> : std::integral_constant<int, kF64> {};
template <> struct DTypeOf<unsigned short> : std::integral_constant<int, kBF16> {};
template <> struct DTypeOf<unsigned char> : std::integral_constant<int, kBool> {};

template <typename T> struct TypeTag { using type = T; };

// f(TypeTag<T>{}) for the T among TS whose code is `dtype`
template <typename... TS, typename F>
int dispatch_dtype(int dtype, F&& f) {
  int rc = kBadArgument;
  (..., (dtype == DTypeOf<TS>::value ? (rc = f(TypeTag<TS>{}), 0) : 0));
  return rc;
}

}  // namespace bk
